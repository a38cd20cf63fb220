// rt_first.hpp -- rt_first_contacts / rt_first_contacts_device: the EARLIEST contact of each of a batch of moving query spheres with the
// scene during one step -- when, with which item, and with what contact normal.  The scene may move too.  What a caller
// that advances bodies asks first: how far can each one go before it touches anything?  rt_swept.hpp's metric, scale and motion table with
// rt_sweep.hpp's shrinking window: one walk, one fixed-size result per query, no count, no scan, no fill.
//
// The time tm of query g against a stream node is rt_swept.hpp's, bit for bit: the same formula on the same S (k_swept_query_magnitude
// folds the queries in by index, whatever the order), the same motion table (enqueue_motion_table), the same dead records, q = 0 a moving
// point, a query whose q is not >= 0 no query at all.
//
// The walk is k_swept_overlaps's loop: thread j carries query order[j] from node 0 in stream order, the node index is wave-uniform (stream
// and motion record arrive through the scalar cache), a lane sleeps while i < resume.  Per lane best = 1, found = false, item = none, and
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
    unsigned gid = blockIdx.x * kBlockThreads + threadIdx.x;
    if (a.order) gid = gid < a.n ? a.order[gid] : kNever;
    const bool in = gid < a.n;
    const size_t g = in ? gid : 0u;
    const T S = impact_scale(*a.magnitude);      // (wave-uniform)
    V3<T> p = { T(0.0), T(0.0), T(0.0) }, dq = { T(0.0), T(0.0), T(0.0) };
    T q = T(0.0);
    constexpr unsigned kNone = 0xFFFFFFFFu;
    unsigned excl = kNone;                       // (an item word's index has 30 bits: kNone and every negative slot match no item)
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
            // k_swept_overlaps's arithmetic; every operation rounded once
            const V3<T> v = { nd.a0 * S - p.x, nd.a1 * S - p.y, nd.a2 * S - p.z };
            const V3<T> w = { dq.x - mo.x, dq.y - mo.y, dq.z - mo.z };
            const T R = mo.E + q;                                    // ((r' + E') + q')
            const T RR = R * R;
            const T qa = dot(w, w), qb = dot(v, w), qc = dot(v, v) - RR;
            const T disc = qb * qb - qa * qc;
            T tm = inf<T>();
            if (nd.a3 > T(0.0)) {
                if (!(qc > T(0.0))) tm = T(0.0);
                else if (qb > T(0.0) && !(disc < T(0.0))) tm = qc / (qb + sqrt_rn_lean(disc));
            }
            const bool beats = found ? tm < best : tm <= best;       // (NaN and +inf never do)
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  inflated by the largest displacement below it
                const bool cull = active && !beats;
                if (cull) resume = nd.skip();
                if (COUNT) c_bounds += active ? 1u : 0u;
                // nobody enters: every lane's resume now lies behind i
                ni = (__ballot(active && !cull) == 0) ? wave_min_u32(resume) : i + 1;
            } else {                                                 // ITEM   the earliest so far
                const bool hit = active && nd.index() != excl && beats;
                if (COUNT) c_items += active ? 1u : 0u;
                if (hit) { best = tm; found = true; win = i; }
                const bool fin = hit && (ANY || tm == T(0.0));       // nothing can beat it (ANY: nothing has to)
                if (fin) resume = kNever;
                ni = (__ballot(fin) != 0) ? wave_min_u32(resume == kNever ? kNever : (resume > i ? resume : i + 1)) : i + 1;
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
                const Motion<T> mo = a.motion[win];
                const V3<T> v = { nd.a0 * S - p.x, nd.a1 * S - p.y, nd.a2 * S - p.z };
                const V3<T> w = { dq.x - mo.x, dq.y - mo.y, dq.z - mo.z };
                u = normalized(V3<T>{ w.x * best - v.x, w.y * best - v.y, w.z * best - v.z });
            }
        }
        if (a.item) a.item[g] = slot != kNone ? (int32_t)slot : -1;
        if (a.normal) {
            T *const out = a.normal + 3 * g;
            out[0] = u.x; out[1] = u.y; out[2] = u.z;
        }
    }
    if constexpr (COUNT) {
        const unsigned long long prim = wave_sum(live ? 1u : 0u), nhit = wave_sum(found ? 1u : 0u);
        const unsigned long long its = wave_sum(c_items), bds = wave_sum(c_bounds);
        if ((threadIdx.x & 63u) == 0u) {
            Counters *const stripe = a.counters + blockIdx.x % kCounterStripes;
            atomicAdd(&stripe->primary, prim);
            atomicAdd(&stripe->hits, nhit);
            atomicAdd(&stripe->sphere_tests, its);
            atomicAdd(&stripe->bound_tests, bds);
        }
    }
}

}  // namespace rt
