// rt_overlap.hpp -- rt_overlap_spheres / rt_overlap_spheres_device: every sphere of the scene that lies within a margin of each query
// sphere, for a batch of query spheres that are NOT items of the scene.  A second set of bodies against a resident world,
// a trigger volume, a sphere about to be spawned.
//
// Query g is {p, q}: a centre and a radius.  For a stream record {c, rr} (rr = the radius squared, rounded once: per_origin_terms,
// rt_skip.hpp), in REAL, every operation rounded once, no FMA contraction, every root correctly rounded (sqrt_rn_lean):
//     v   = c - p
//     vv  = (v.x*v.x + v.y*v.y) + v.z*v.z                                     dot()'s order
//     gap = rr > 0 ? (sqrt(vv) - sqrt(rr)) - q : +inf
// rt_near.hpp's gap minus the query's radius -- rt_contacts.hpp's gap with q given by the caller instead of taken from the stream; with
// q = 0 it is rt_near.hpp's bit for bit (x - 0 == x).  An item is LISTED when !(gap >= margin), a bound CULLS when gap >= margin (a bound
// without a positive rr: always).  A query whose q is not >= 0 (negative, NaN) carries no query: no test, nothing listed.  The dead record
// of DESIGN.md 4.13 is {0, 0, 0, -inf}: a dead item is at +inf -- never listed -- and a dead BOUND culls for every query.
//
// The walk is made of rt_walk.hpp's pieces (lane_query, centre_gap, bound_step_min) over the whole stream from node 0: one query per lane,
// a lane sleeps while i < resume, a lane whose own bound test culls a subtree sets resume = skip.  When no awake lane enters a bound the
// wave continues at the smallest resume of its lanes, as k_contact_pairs does; a wave none of whose lanes carries a query never enters
// the loop.  The query's `exclude` slot is tested and counted as a test, but never listed.
//
// The list is rt_contacts.hpp's: the walk runs twice.  The first pass writes one count per query; the exclusive scan of rt_contacts.hpp
// turns the counts into offsets; the second pass repeats the walk and writes entry offsets[g] + (rank within g) where that lies below the
// capacity.  Entries are sorted by (g, item slot) by construction, and a capacity that is too small gets the exact prefix.  In the second
// pass a lane whose query counted nothing has nothing to write and carries no query: a wave of such lanes returns at once, and the others
// walk without them.
#pragma once
#include "rt_contacts.hpp"

namespace rt {

template <typename T> struct OverlapArgs {
    const Node<T> *stream;          // plain per-origin stream, END-padded
    const T *queries;               // [4 n]: p.x, p.y, p.z, q
    const int32_t *exclude;         // [n] or NULL: the item slot query g never lists (-1, or any slot outside the scene: none)
    const uint32_t *order;          // [n] or NULL: thread j carries query order[j]; an entry >= n carries none
    uint32_t *counts;               // [n]: written by the first pass, read by FILL
    const uint64_t *offsets;        // FILL: [n + 1], the exclusive scan of counts
    int32_t *items;                 // FILL: [capacity]
    T *gap;                         // FILL: [capacity] or NULL
    Counters *counters;             // COUNT: kCounterStripes slots
    T margin;
    uint32_t n_nodes;               // nodes in front of END
    uint32_t n;                     // queries
    uint32_t capacity;              // FILL: entries the caller has room for
};

template <typename T, bool COUNT, bool FILL>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_overlap_spheres(OverlapArgs<T> a)
{
    static_assert(!(COUNT && FILL), "the counters are the first pass's");
    const unsigned gid = lane_query(a.order != nullptr, a.order, a.n);
    const bool in = gid < a.n;
    const size_t g = in ? gid : 0u;
    V3<T> p = { T(0.0), T(0.0), T(0.0) };
    T q = T(0.0);
    unsigned excl = kNone;
    unsigned resume = kNever;                    // a lane without a query never wakes
    unsigned long long at = 0;                   // FILL: where query g's entries start
    if (in) {
        const T *const rec = a.queries + 4 * g;
        q = rec[3];
        bool carries = q >= T(0.0);              // (NaN fails the comparison)
        if (FILL) carries = carries && a.counts[g] != 0u;            // nothing to write: no walk
        if (carries) {
            p = { rec[0], rec[1], rec[2] };
            if (a.exclude) excl = (unsigned)a.exclude[g];
            if (FILL) at = a.offsets[g];
            resume = 0u;
        }
    }
    const bool live = resume != kNever;
    const T margin = a.margin;
    unsigned found = 0;
    unsigned c_items = 0, c_bounds = 0;
    const unsigned n = a.n_nodes;
    const unsigned first = wave_min_u32(resume);                     // 0, or kNever: no lane of the wave carries a query
    if (first < n) {
        unsigned i = (unsigned)__builtin_amdgcn_readfirstlane((int)first);
        Node<T> nd = a.stream[i];
        for (;;) {
            const bool active = i >= resume;
            const T t = centre_gap(nd, p, q);                        // the gap above
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  against the margin
                const bool cull = active && (t >= margin);
                ni = bound_step_min<COUNT>(active, cull, nd, i, resume, c_bounds);
            } else {                                                 // ITEM   within the margin of the lane's sphere
                const unsigned it = nd.index();
                const bool hit = active && it != excl && !(t >= margin);
                if (FILL) {
                    const unsigned long long pos = at + found;
                    if (hit && pos < (unsigned long long)a.capacity) {
                        a.items[pos] = (int32_t)it;
                        if (a.gap) a.gap[pos] = t;
                    }
                }
                found += hit ? 1u : 0u;
                if (COUNT) c_items += active ? 1u : 0u;
                ni = i + 1;
            }
            if (ni >= n) break;                                      // also kNever: every lane is done
            i = (unsigned)__builtin_amdgcn_readfirstlane((int)ni);
            nd = a.stream[i];
        }
    }
    if (!FILL && in) a.counts[g] = found;
    if constexpr (COUNT)
        flush_counters(a.counters, wave_sum(live ? 1u : 0u), wave_sum((live && found > 0u) ? 1u : 0u), wave_sum(c_items), wave_sum(c_bounds));
}

}  // namespace rt
