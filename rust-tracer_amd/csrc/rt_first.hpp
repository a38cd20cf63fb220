// rt_first.hpp -- rt_first_contacts / rt_first_contacts_device: the EARLIEST contact of each of a batch of moving query spheres with the
// scene during one step -- when, with which item, and with what contact normal.  The scene may move too.  What a caller
// that advances bodies asks first: how far can each one go before it touches anything?  rt_swept.hpp's metric, scale and motion table with
// rt_sweep.hpp's shrinking window: one walk, one fixed-size result per query, no count, no scan, no fill.
//
// The time tm of query g against a stream node is rt_swept.hpp's, bit for bit: the same formula on the same S (k_swept_query_magnitude
// folds the queries in by index, whatever the order), the same motion table (enqueue_motion_table), the same dead records, q = 0 a moving
// point, a query whose q is not >= 0 no query at all.
//
// The walk is built as k_swept_overlaps's is, from rt_walk.hpp's pieces (lane_query, swept_time, bound_step_min, and item_step_retire for
// a lane that is finished): thread j carries query order[j] from node 0 in stream order, stream and motion record arrive through the
// scalar cache, a lane sleeps while i < resume.  Per lane best = 1, found = false, item = none, and
// ONE predicate serves both kinds of node:
//     beats(tm) = found ? tm < best : tm <= best
// A BOUND is entered when beats, else culled to its skip.  An ITEM whose slot is not the lane's `exclude` and that beats becomes the
// result: best = tm, found = true.  The excluded item is tested and counted, and never becomes the result.  On a tie the first item in
// stream order wins (item slots are DFS order: the lowest slot); a contact at exactly t = 1 is found, and a later one at t = 1 does not
// replace it.  The lane is finished (resume = kNever) as soon as found && best == 0 -- nothing beats a start in contact -- and, ANY, as
// soon as found.  The result is the walk's, as for every query here.  NaN and +inf never beat, the index only grows, and every index is
// used behind a comparison: the walk ends whatever bits the queries carry.
//
// The loop keeps the winning NODE's index besides the time; the normal -- rt_swept.hpp's u = w * t - v, normalized -- is formed once
// behind the loop from that node's two records, by the loop's own expressions: the same bits at no cost inside the loop.
#pragma once
#include "rt_swept.hpp"

namespace rt {

template <typename T> struct FirstArgs {
    const Node<T> *stream;          // plain per-origin stream, END-padded
    const Motion<T> *motion;        // [n_nodes], parallel to the stream
    const T *magnitude;             // M of this call: the scene's, its displacements' and the queries'
    const T *queries;               // [4 n]: p.x, p.y, p.z, q
    const T *qdisp;                 // [3 n]: dq
    const int32_t *exclude;         // [n] or NULL: the item slot query g never returns (-1, or any slot outside the scene: none)
    const uint32_t *order;          // [n] or NULL: thread j carries query order[j]; an entry >= n carries none
    T *time;                        // [n]: best, or +inf
    int32_t *item;                  // [n] or NULL: the slot, or -1
    T *normal;                      // [3 n] or NULL: the normal at best, or {0, 0, 0}
    Counters *counters;             // COUNT: kCounterStripes slots
    uint32_t n_nodes;               // nodes in front of END
    uint32_t n;                     // queries
};

// The motion record of wave-uniform node i, asked for NEXT TO the stream record.  Left alone, the compiler sinks this load into the
// branch that first uses it (a live node), behind the wait for the stream record: two scalar round trips a step, one after the other.
// A readfirstlane of every word -- a plain copy for a value that already is wave-uniform -- is not moved across control flow, and keeps
// the load where it is written; both records are then in flight at once.
template <typename T>
__device__ __forceinline__ Motion<T> motion_alongside(const Motion<T> *motion, unsigned i)
{
    constexpr int kWords = (int)(sizeof(Motion<T>) / sizeof(int));
    Motion<T> mo = motion[i];
    int w[kWords];
    __builtin_memcpy(w, &mo, sizeof mo);
#pragma unroll
    for (int k = 0; k < kWords; ++k) w[k] = __builtin_amdgcn_readfirstlane(w[k]);
    __builtin_memcpy(&mo, w, sizeof mo);
    return mo;
}

template <typename T, bool COUNT, bool ANY>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_first_contacts(FirstArgs<T> a)
{
    const unsigned gid = lane_query(a.order != nullptr, a.order, a.n);
    const bool in = gid < a.n;
    const size_t g = in ? gid : 0u;
    const T S = impact_scale(*a.magnitude);      // (wave-uniform)
    V3<T> p = { T(0.0), T(0.0), T(0.0) }, dq = { T(0.0), T(0.0), T(0.0) };
    T q = T(0.0);
    unsigned excl = kNone;
    unsigned resume = kNever;                    // a lane without a query never wakes
    if (in) {
        const T *const rec = a.queries + 4 * g;
        const T radius = rec[3];
        if (radius >= T(0.0)) {                  // (NaN fails the comparison)
            const T *const mv = a.qdisp + 3 * g;
            p = { rec[0] * S, rec[1] * S, rec[2] * S };
            dq = { mv[0] * S, mv[1] * S, mv[2] * S };
            q = radius * S;
            if (a.exclude) excl = (unsigned)a.exclude[g];
            resume = 0u;
        }
    }
    const bool live = resume != kNever;
    T best = T(1.0);
    bool found = false;
    unsigned win = 0;                            // found: the node that gave best
    unsigned c_items = 0, c_bounds = 0;
    const unsigned n = a.n_nodes;
    const unsigned first = wave_min_u32(resume);                     // 0, or kNever: no lane of the wave carries a query
    if (first < n) {
        unsigned i = (unsigned)__builtin_amdgcn_readfirstlane((int)first);
        Node<T> nd = a.stream[i];
        Motion<T> mo = motion_alongside(a.motion, i);
        for (;;) {
            const bool active = i >= resume;
            V3<T> v, w;
            const T tm = swept_time(nd, mo, S, p, dq, q, v, w);      // k_swept_overlaps's
            const bool beats = found ? tm < best : tm <= best;       // (NaN and +inf never do)
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  inflated by the largest displacement below it
                const bool cull = active && !beats;
                ni = bound_step_min<COUNT>(active, cull, nd, i, resume, c_bounds);
            } else {                                                 // ITEM   the earliest so far
                const bool hit = active && nd.index() != excl && beats;
                if (COUNT) c_items += active ? 1u : 0u;
                if (hit) { best = tm; found = true; win = i; }
                const bool fin = hit && (ANY || tm == T(0.0));       // nothing can beat it (ANY: nothing has to)
                ni = item_step_retire(fin, i, resume);
            }
            if (ni >= n) break;                                      // also kNever: every lane is done
            i = (unsigned)__builtin_amdgcn_readfirstlane((int)ni);
            nd = a.stream[i];
            mo = motion_alongside(a.motion, i);
        }
    }
    if (in) {
        a.time[g] = found ? best : inf<T>();
        V3<T> u = { T(0.0), T(0.0), T(0.0) };
        unsigned slot = kNone;
        if (found && win < n) {                                      // (win is a node the loop stood on)
            const Node<T> nd = a.stream[win];
            slot = nd.index();
            if (a.normal) {                                          // the loop's v and w of that node, then rt_swept.hpp's normal
                V3<T> v, w;
                swept_frame(nd, a.motion[win], S, p, dq, v, w);
                u = swept_normal(v, w, best);
            }
        }
        if (a.item) a.item[g] = slot != kNone ? (int32_t)slot : -1;
        if (a.normal) {
            T *const out = a.normal + 3 * g;
            out[0] = u.x; out[1] = u.y; out[2] = u.z;
        }
    }
    if constexpr (COUNT)
        flush_counters(a.counters, wave_sum(live ? 1u : 0u), wave_sum(found ? 1u : 0u), wave_sum(c_items), wave_sum(c_bounds));
}

}  // namespace rt
