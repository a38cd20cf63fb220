// rt_swept.hpp -- rt_swept_overlaps / rt_swept_overlaps_device: every sphere of the scene that each of a batch of MOVING query spheres
// comes into contact with during one step, when, and with what contact normal.  The queries are NOT items of the scene --
// particles against level geometry, another scene's spheres, a projectile, a swept trigger volume -- and the scene may move too.
// rt_overlap.hpp's walk and list with rt_impacts.hpp's metric, scale and motion table.
//
// Query g is {p, q} (queries[4g .. 4g+4]) and moves by dq (qdisp[3g .. 3g+3]): it is at p + t dq for t in [0, 1].  For a stream node with
// record {c, rr} and motion record {e', r' + E'} (rt_impacts.hpp's table, made for this call's `disp` and S), in REAL, every operation
// rounded once, no FMA contraction, every root correctly rounded (sqrt_rn_lean), every dot product dot()'s:
//     p' = p S    q' = q S    dq' = dq S                         c', r', d', E' as in rt_impacts.hpp
//     v = c' - p'        w = dq' - e'         R = (r' + E') + q'      RR = R * R
//     a = dot(w, w)   b = dot(v, w)   cc = dot(v, v) - RR   disc = b*b - a*cc
//     t = +inf                       if !(rr > 0)
//       = 0                          else if !(cc > 0)              in contact at the start
//       = +inf                       else if !(b > 0) or disc < 0   not approaching (w = 0 too), or passing by
//       = cc / (b + sqrt(disc))      otherwise
// rt_impacts.hpp's formula with the query in the place of item i.  An item is LISTED when t <= 1, a bound CULLS when !(t <= 1).  A query
// whose q is not >= 0 (negative, NaN) carries no query; q = 0 is a moving point.  The `exclude` slot is tested and counted as a test, never
// listed.  The NORMAL of an entry is normalized(u), u = {w.x*t - v.x, w.y*t - v.y, w.z*t - v.z} (each product and difference rounded
// once): the query's centre minus the touched sphere's centre at time t, in the scaled frame -- from the touched sphere to the query, as
// rt_sweep.hpp has it.  Coincident centres at t = 0 give u = 0 and normalized() then gives 0 * (1 / 0) = NaN in all three components.
//
// S is rt_impacts.hpp's with the queries folded into M: k_swept_query_magnitude takes the largest of |p.x|, |p.y|, |p.z|, q, |dq.x|, |dq.y|,
// |dq.z| over every query with q >= 0 -- by query index, whatever the order -- into the magnitude word the motion kernels fold the scene
// into (atomic_max_bits: max is exact, the word is the same every time).  It runs before k_impact_motion_bounds, which reads S.
//
// The walk is built as k_overlap_spheres's is, from rt_walk.hpp's pieces (lane_query; swept_time, the formula above): thread j carries
// query order[j] from node 0, stream and motion record arrive through the scalar cache, a lane sleeps while i < resume, the wave goes to
// the smallest resume when nobody enters, a wave without a query returns before the loop, and in the FILL pass a query whose count is 0
// carries no query.  The BOUND step and the normal stand in this kernel's own text: called from here, rt_walk.hpp's bound_step_min and
// swept_normal made the counting and the FILL flavours two to three instructions longer.  Count pass, rt_contacts.hpp's
// scan, fill pass: the list is sorted by (g, item slot) and the same bytes every time.
#pragma once
#include "rt_impacts.hpp"

namespace rt {

template <typename T> struct SweptArgs {
    const Node<T> *stream;          // plain per-origin stream, END-padded
    const Motion<T> *motion;        // [n_nodes], parallel to the stream
    const T *magnitude;             // M of this call: the scene's, its displacements' and the queries'
    const T *queries;               // [4 n]: p.x, p.y, p.z, q
    const T *qdisp;                 // [3 n]: dq
    const int32_t *exclude;         // [n] or NULL: the item slot query g never lists (-1, or any slot outside the scene: none)
    const uint32_t *order;          // [n] or NULL: thread j carries query order[j]; an entry >= n carries none
    uint32_t *counts;               // [n]: written by the first pass, read by FILL
    const uint64_t *offsets;        // FILL: [n + 1], the exclusive scan of counts
    int32_t *items;                 // FILL: [capacity]
    T *time;                        // FILL: [capacity] or NULL
    T *normal;                      // FILL: [3 capacity] or NULL
    Counters *counters;             // COUNT: kCounterStripes slots
    uint32_t n_nodes;               // nodes in front of END
    uint32_t n;                     // queries
    uint32_t capacity;              // FILL: entries the caller has room for
};

// The queries' part of M.  Thread g looks at query g; the caller has set *magnitude to 0 (or the motion kernels have folded into it: max
// commutes).
template <typename T>
__global__ __launch_bounds__(256) void k_swept_query_magnitude(const T *__restrict__ queries, const T *__restrict__ qdisp, unsigned n, T *__restrict__ magnitude)
{
    __shared__ T part[4];
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    T m = T(0.0);
    if (g < n) {
        const T *const rec = queries + 4 * (size_t)g;
        const T *const dq = qdisp + 3 * (size_t)g;
        const T q = rec[3];
        if (q >= T(0.0))                                             // (NaN fails the comparison: no query)
            m = max_rn(max_rn(max_rn(abs_rn(rec[0]), abs_rn(rec[1])), max_rn(abs_rn(rec[2]), q)), max_rn(max_rn(abs_rn(dq[0]), abs_rn(dq[1])), abs_rn(dq[2])));
    }
    m = wave_max_real(m);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const T all = max_rn(max_rn(part[0], part[1]), max_rn(part[2], part[3]));
        if (all > T(0.0)) atomic_max_bits(magnitude, all);
    }
}

template <typename T, bool COUNT, bool FILL>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_swept_overlaps(SweptArgs<T> a)
{
    static_assert(!(COUNT && FILL), "the counters are the first pass's");
    const unsigned gid = lane_query(a.order != nullptr, a.order, a.n);
    const bool in = gid < a.n;
    const size_t g = in ? gid : 0u;
    const T S = impact_scale(*a.magnitude);      // (wave-uniform)
    V3<T> p = { T(0.0), T(0.0), T(0.0) }, dq = { T(0.0), T(0.0), T(0.0) };
    T q = T(0.0);
    unsigned excl = kNone;
    unsigned resume = kNever;                    // a lane without a query never wakes
    unsigned long long at = 0;                   // FILL: where query g's entries start
    if (in) {
        const T *const rec = a.queries + 4 * g;
        const T radius = rec[3];
        bool carries = radius >= T(0.0);         // (NaN fails the comparison)
        if (FILL) carries = carries && a.counts[g] != 0u;            // nothing to write: no walk
        if (carries) {
            const T *const mv = a.qdisp + 3 * g;
            p = { rec[0] * S, rec[1] * S, rec[2] * S };
            dq = { mv[0] * S, mv[1] * S, mv[2] * S };
            q = radius * S;
            if (a.exclude) excl = (unsigned)a.exclude[g];
            if (FILL) at = a.offsets[g];
            resume = 0u;
        }
    }
    const bool live = resume != kNever;
    unsigned found = 0;
    unsigned c_items = 0, c_bounds = 0;
    const unsigned n = a.n_nodes;
    const unsigned first = wave_min_u32(resume);                     // 0, or kNever: no lane of the wave carries a query
    if (first < n) {
        unsigned i = (unsigned)__builtin_amdgcn_readfirstlane((int)first);
        Node<T> nd = a.stream[i];
        Motion<T> mo = a.motion[i];
        for (;;) {
            const bool active = i >= resume;
            V3<T> v, w;
            const T tm = swept_time(nd, mo, S, p, dq, q, v, w);      // k_impact_pairs's, with the lane's query in the place of item i
            const bool within = tm <= T(1.0);
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  inflated by the largest displacement below it
                const bool cull = active && !within;
                if (cull) resume = nd.skip();
                if (COUNT) c_bounds += active ? 1u : 0u;
                // nobody enters: every lane's resume now lies behind i
                ni = (__ballot(active && !cull) == 0) ? wave_min_u32(resume) : i + 1;
            } else {                                                 // ITEM   touched by the lane's sphere during the step
                const unsigned it = nd.index();
                const bool hit = active && it != excl && within;
                if (FILL) {
                    const unsigned long long pos = at + found;
                    if (hit && pos < (unsigned long long)a.capacity) {
                        a.items[pos] = (int32_t)it;
                        if (a.time) a.time[pos] = tm;
                        if (a.normal) {
                            const V3<T> u = normalized(V3<T>{ w.x * tm - v.x, w.y * tm - v.y, w.z * tm - v.z });
                            T *const out = a.normal + 3 * pos;
                            out[0] = u.x; out[1] = u.y; out[2] = u.z;
                        }
                    }
                }
                found += hit ? 1u : 0u;
                if (COUNT) c_items += active ? 1u : 0u;
                ni = i + 1;
            }
            if (ni >= n) break;                                      // also kNever: every lane is done
            i = (unsigned)__builtin_amdgcn_readfirstlane((int)ni);
            nd = a.stream[i];
            mo = a.motion[i];
        }
    }
    if (!FILL && in) a.counts[g] = found;
    if constexpr (COUNT)
        flush_counters(a.counters, wave_sum(live ? 1u : 0u), wave_sum((live && found > 0u) ? 1u : 0u), wave_sum(c_items), wave_sum(c_bounds));
}

}  // namespace rt
