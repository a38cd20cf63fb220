// rt_box.hpp -- rt_overlap_boxes / rt_overlap_boxes_device: every sphere of the scene that lies within a margin of each query BOX, for a
// batch of axis-aligned boxes.  A trigger or kill volume, a selection rectangle, the broad-phase box of a body that is no
// sphere, a grid cell; with infinite sides a slab or a half-space ("everything below this floor").
//
// Query g is {lo, hi}: two corners.  For a stream record {c, rr} (rr = the radius squared, rounded once: per_origin_terms, rt_skip.hpp),
// in REAL, every operation rounded once, no FMA contraction, every root correctly rounded (sqrt_rn_lean), per axis k:
//     e_k = lo_k - c_k
//     f_k = c_k - hi_k
//     e_k = f_k > e_k ? f_k : e_k
//     e_k = e_k > 0 ? e_k : 0                                                 comparisons, not fmax
//     dd  = (e.x*e.x + e.y*e.y) + e.z*e.z                                     dot()'s order
//     gap = rr > 0 ? sqrt(dd) - sqrt(rr) : +inf
// the distance from the box to the sphere's SURFACE, floored at -r: a centre inside the box has gap = -r however deep it lies -- this is no
// signed depth.  An item is LISTED when !(gap >= margin), a bound CULLS when gap >= margin (a bound without a positive rr: always).  A box
// carries a query exactly when lo_k <= hi_k on all three axes (NaN fails the comparison): an inverted box makes no test and lists
// nothing.  Infinite sides are valid (lo = -inf, hi = +inf): no step above makes a NaN from them.  A point box lo == hi == p gives
// rt_overlap.hpp's gap with q = 0 bit for bit (lo - c and c - hi are exact negatives of each other, and x - 0 == x).  The dead record of
// DESIGN.md 4.13 is {0, 0, 0, -inf}: a dead item is at +inf -- never listed -- and a dead BOUND culls for every box.
//
// The walk is k_overlap_spheres's, made of rt_walk.hpp's pieces (lane_query, box_gap, bound_step_min) over the whole stream from node 0:
// one box per lane, six reals where k_overlap_spheres carries four; a lane sleeps while i < resume, a lane whose own bound test culls a
// subtree sets resume = skip.  When no awake lane enters a bound the wave continues at the smallest resume of its lanes; a wave none of
// whose lanes carries a query never enters the loop.  The box's `exclude` slot is tested and counted as a test, but never listed.
//
// The list is rt_contacts.hpp's, in rt_overlap.hpp's workspace: the walk runs twice.  The first pass writes one count per box; the
// exclusive scan of rt_contacts.hpp turns the counts into offsets; the second pass repeats the walk and writes entry offsets[g] + (rank
// within g) where that lies below the capacity.  Entries are sorted by (g, item slot) by construction, and a capacity that is too small
// gets the exact prefix.  In the second pass a lane whose box counted nothing has nothing to write and carries no query.
#pragma once
#include "rt_contacts.hpp"

namespace rt {

template <typename T> struct BoxArgs {
    const Node<T> *stream;          // plain per-origin stream, END-padded
    const T *boxes;                 // [6 n]: lo.x, lo.y, lo.z, hi.x, hi.y, hi.z
    const int32_t *exclude;         // [n] or NULL: the item slot box g never lists (-1, or any slot outside the scene: none)
    const uint32_t *order;          // [n] or NULL: thread j carries box order[j]; an entry >= n carries none
    uint32_t *counts;               // [n]: written by the first pass, read by FILL
    const uint64_t *offsets;        // FILL: [n + 1], the exclusive scan of counts
    int32_t *items;                 // FILL: [capacity]
    T *gap;                         // FILL: [capacity] or NULL
    Counters *counters;             // COUNT: kCounterStripes slots
    T margin;
    uint32_t n_nodes;               // nodes in front of END
    uint32_t n;                     // boxes
    uint32_t capacity;              // FILL: entries the caller has room for
};

template <typename T, bool COUNT, bool FILL>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_overlap_boxes(BoxArgs<T> a)
{
    static_assert(!(COUNT && FILL), "the counters are the first pass's");
    const unsigned gid = lane_query(a.order != nullptr, a.order, a.n);
    const bool in = gid < a.n;
    const size_t g = in ? gid : 0u;
    V3<T> lo = { T(0.0), T(0.0), T(0.0) }, hi = { T(0.0), T(0.0), T(0.0) };
    unsigned excl = kNone;
    unsigned resume = kNever;                    // a lane without a query never wakes
    unsigned long long at = 0;                   // FILL: where box g's entries start
    if (in) {
        const T *const rec = a.boxes + 6 * g;
        const V3<T> l = { rec[0], rec[1], rec[2] }, h = { rec[3], rec[4], rec[5] };
        bool carries = l.x <= h.x && l.y <= h.y && l.z <= h.z;       // (NaN fails the comparison)
        if (FILL) carries = carries && a.counts[g] != 0u;            // nothing to write: no walk
        if (carries) {
            lo = l;
            hi = h;
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
            const T t = box_gap(nd, lo, hi);                         // the gap above
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  against the margin
                const bool cull = active && (t >= margin);
                ni = bound_step_min<COUNT>(active, cull, nd, i, resume, c_bounds);
            } else {                                                 // ITEM   within the margin of the lane's box
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
