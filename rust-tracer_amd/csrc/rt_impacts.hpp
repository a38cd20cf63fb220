// rt_impacts.hpp -- rt_scene_impacts / rt_scene_impacts_device: every pair of spheres of the scene that comes into contact during one step,
// and when.  The continuous collision step of a particle caller: rt_contacts.hpp's self-join with rt_sweep.hpp's cast as
// its metric, both spheres moving.
//
// For two item slots i < j with stream records {c_i, rr_i} and {c_j, rr_j} and displacements d_i, d_j (sphere k is at c_k + t d_k for t in
// [0, 1]), in REAL, every operation rounded once, no FMA contraction, every root correctly rounded (sqrt_rn_lean), every dot product dot()'s:
//     v = c_j - c_i            w = d_i - d_j                     the lower slot is the query
//     R = (sqrt(rr_j) + E) + sqrt(rr_i)       RR = R * R         E = 0 for an item
//     a = dot(w, w)    b = dot(v, w)    c = dot(v, v) - RR       disc = b*b - a*c
//     t = +inf                     if !(rr_i > 0 && rr_j > 0)
//       = 0                        else if !(c > 0)              in contact at the start
//       = +inf                     else if !(b > 0) or disc < 0  not approaching (w = 0 too), or passing by
//       = c / (b + sqrt(disc))     otherwise                     the smaller root of a t^2 - 2 b t + c = 0, without a division by a
// (i, j) is an IMPACT when t <= 1.
//
// A bound {C, RRn} that encloses its items at the start of the step encloses them during all of it once its radius grows by the largest
// displacement below it.  The MOTION TABLE, one record {e.x, e.y, e.z, E} per stream node, carries that: an ITEM node of slot j holds
// {d_j, 0}, a BOUND node {0, 0, 0, D} with D = max m_j * (1 + kRefitK eps) over the live items of its subtree -- the stream range (node,
// skip) -- and m_j the length of d_j by the refit's rule (rt_dynamic.hpp): sqrt(s) where s = dot(d_j, d_j) >= refit_tiny, else |dx| + |dy|
// + |dz|; 0 for a record without a positive rr.  The walk then applies ONE formula to every node, w = d_i - e and E as stored: for an item
// that is the definition bit for bit, for a bound the cast of the query (its own motion stays in w) against a standing sphere of radius
// r + D.  A lane culls a bound's subtree when !(t <= 1).
//
// The table is made per call: k_impact_motion_items writes the item records and every node's length m (0 for a bound) and folds the lengths
// of kMotionChunk consecutive nodes into one maximum; k_impact_motion_bounds gives a wave 64 consecutive nodes, and for each bound among
// them the wave folds the range (node, skip): single lengths up to the first chunk boundary, whole chunks, single lengths behind the last
// boundary.  max is exact, so the split cannot show in the bytes.
//
// The walk is k_contact_pairs's (rt_contacts.hpp): lane t carries item slot t and walks only the stream behind its own node, the node index
// is wave-uniform (node and motion record arrive through the scalar cache), and the wave continues at the smallest resume when nobody
// enters.  Count pass, rt_contacts.hpp's scan, fill pass: the list is sorted by (i, j) and the same bytes every time.
#pragma once
#include "rt_contacts.hpp"
#include "rt_dynamic.hpp"

namespace rt {

template <typename T> struct alignas(sizeof(T) * 4) Motion { T x, y, z, E; };
static_assert(sizeof(Motion<float>) == 16 && sizeof(Motion<double>) == 32, "motion records are one aligned scalar-load unit");

constexpr unsigned kMotionChunk = 256;             // node lengths per chunk maximum: one block of k_impact_motion_items

template <typename T> struct ImpactArgs {
    const Node<T> *stream;          // plain per-origin stream, END-padded
    const Motion<T> *motion;        // [n_nodes], parallel to the stream
    const uint32_t *item_node;      // [n_items]: the node of every item slot, or NULL: item t is node t (a scene without bounds)
    uint32_t *counts;               // first pass: [n_items], the impacts item t has as the lower slot
    const uint64_t *offsets;        // FILL: [n_items + 1], the exclusive scan of counts
    int32_t *pairs;                 // FILL: [2 capacity]
    T *time;                        // FILL: [capacity] or NULL
    Counters *counters;             // COUNT: kCounterStripes slots
    uint32_t n_nodes;               // nodes in front of END
    uint32_t n_items;
    uint32_t capacity;              // FILL: pairs the caller has room for
};

template <typename T, bool COUNT, bool FILL>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_impact_pairs(ImpactArgs<T> a)
{
    static_assert(!(COUNT && FILL), "the counters are the first pass's");
    const unsigned t = blockIdx.x * kBlockThreads + threadIdx.x;
    const bool in = t < a.n_items;
    V3<T> p = { T(0.0), T(0.0), T(0.0) }, d = { T(0.0), T(0.0), T(0.0) };
    T q = T(0.0);
    unsigned resume = kNever;                    // a lane without a live item never wakes
    if (in) {
        const unsigned node = a.item_node ? a.item_node[t] : t;
        const unsigned at_node = node < a.n_nodes ? node : 0u;
        const Node<T> *const me = a.stream + at_node;
        const T rr = me->a3;
        if (node < a.n_nodes && rr > T(0.0)) {                       // (a slot the stream does not hold has no node: no query)
            const Motion<T> mine = a.motion[at_node];
            p = { me->a0, me->a1, me->a2 };
            d = { mine.x, mine.y, mine.z };
            q = sqrt_rn_lean(rr);
            resume = node + 1u;
        }
    }
    const bool live = resume != kNever;
    unsigned long long at = 0;                   // FILL: where item t's pairs start
    if (FILL) at = live ? a.offsets[t] : 0ull;
    unsigned found = 0;
    unsigned c_items = 0, c_bounds = 0;
    const unsigned n = a.n_nodes;
    const unsigned first = wave_min_u32(resume);
    if (first < n) {
        unsigned i = (unsigned)__builtin_amdgcn_readfirstlane((int)first);
        Node<T> nd = a.stream[i];
        Motion<T> mo = a.motion[i];
        for (;;) {
            const bool active = i >= resume;
            // the definition above, one formula for both kinds of node; every operation rounded once
            const V3<T> v = { nd.a0 - p.x, nd.a1 - p.y, nd.a2 - p.z };
            const V3<T> w = { d.x - mo.x, d.y - mo.y, d.z - mo.z };
            const T R = (sqrt_rn_lean(nd.a3) + mo.E) + q;
            const T RR = R * R;
            const T qa = dot(w, w), qb = dot(v, w), qc = dot(v, v) - RR;
            const T disc = qb * qb - qa * qc;
            T tm = inf<T>();
            if (nd.a3 > T(0.0)) {
                if (!(qc > T(0.0))) tm = T(0.0);
                else if (qb > T(0.0) && !(disc < T(0.0))) tm = qc / (qb + sqrt_rn_lean(disc));
            }
            const bool within = tm <= T(1.0);
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  inflated by the largest displacement below it
                const bool cull = active && !within;
                if (cull) resume = nd.skip();
                if (COUNT) c_bounds += active ? 1u : 0u;
                // nobody enters: every lane's resume now lies behind i -- the skip target, or a sleeping lane's own start inside the subtree
                ni = (__ballot(active && !cull) == 0) ? wave_min_u32(resume) : i + 1;
            } else {                                                 // ITEM   an impact of the lane's item with a later one
                const bool hit = active && within;
                if (FILL) {
                    const unsigned long long pos = at + found;
                    if (hit && pos < (unsigned long long)a.capacity) {
                        a.pairs[2 * pos] = (int32_t)t;
                        a.pairs[2 * pos + 1] = (int32_t)nd.index();
                        if (a.time) a.time[pos] = tm;
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
    if (!FILL && in) a.counts[t] = found;
    if constexpr (COUNT) {
        const unsigned long long prim = wave_sum(live ? 1u : 0u), nhit = wave_sum((live && found > 0u) ? 1u : 0u);
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

// ---- the motion table ----

template <typename T> __device__ __forceinline__ T wave_max_real(T v)
{
    for (int off = 32; off > 0; off >>= 1) v = max_rn(v, __shfl_xor(v, off, 64));
    return v;
}

// Thread i looks at node i: an ITEM node of slot j takes {d_j, 0} and the length m_j (0 without a positive rr), a BOUND node the length 0
// (its record is k_impact_motion_bounds's).  Block b leaves the largest length of its kMotionChunk nodes in chunk[b].
template <typename T>
__global__ __launch_bounds__(kMotionChunk) void k_impact_motion_items(const Node<T> *__restrict__ stream, const T *__restrict__ disp, unsigned n_nodes, unsigned n_items,
                                                                      Motion<T> *__restrict__ motion, T *__restrict__ length, T *__restrict__ chunk)
{
    __shared__ T part[kMotionChunk / 64];
    const unsigned i = blockIdx.x * kMotionChunk + threadIdx.x;
    T m = T(0.0);
    if (i < n_nodes) {
        const uint32_t word = stream[i].item;
        const uint32_t slot = word & kNodeIndexMask;
        if ((word & kNodeItem) != 0u && (word & kNodeEnd) == 0u && slot < n_items) {
            const T dx = disp[3 * (size_t)slot], dy = disp[3 * (size_t)slot + 1], dz = disp[3 * (size_t)slot + 2];
            motion[i] = { dx, dy, dz, T(0.0) };
            if (stream[i].a3 > T(0.0)) {
                const T s = (dx * dx + dy * dy) + dz * dz;
                m = s >= refit_tiny<T>() ? sqrt_rn_lean(s) : (abs_rn(dx) + abs_rn(dy)) + abs_rn(dz);
            }
        } else {
            motion[i] = { T(0.0), T(0.0), T(0.0), T(0.0) };              // (a BOUND's record is rewritten by k_impact_motion_bounds; no node is left undefined)
        }
        length[i] = m;
    }
    m = wave_max_real(m);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        T all = part[0];
        for (unsigned k = 1; k < kMotionChunk / 64; ++k) all = max_rn(all, part[k]);
        chunk[blockIdx.x] = all;
    }
}

// One wave per 64 consecutive nodes; for every BOUND among them the whole wave folds the lengths of the stream range (node, skip).
template <typename T>
__global__ __launch_bounds__(256) void k_impact_motion_bounds(const Node<T> *__restrict__ stream, unsigned n_nodes, const T *__restrict__ length,
                                                              const T *__restrict__ chunk, Motion<T> *__restrict__ motion)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned base = (blockIdx.x * 256u + threadIdx.x) - lane;
    if (base >= n_nodes) return;                                     // (wave-uniform)
    const unsigned i = base + lane;
    bool bound = false;
    unsigned skip = 0;
    if (i < n_nodes) {
        const Node<T> *const nd = stream + i;
        bound = (nd->item & (kNodeItem | kNodeEnd)) == 0u;
        skip = nd->skip_off / (unsigned)sizeof(Node<T>);
    }
    unsigned long long todo = __ballot(bound);
    while (todo != 0ull) {
        const unsigned k = (unsigned)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const unsigned lo = base + k + 1u;
        unsigned hi = (unsigned)__shfl((int)skip, (int)k, 64);
        if (hi > n_nodes) hi = n_nodes;
        // [lo, head): single lengths; [head, tail): whole chunks; [tail, hi): single lengths
        unsigned head = (lo + kMotionChunk - 1u) / kMotionChunk * kMotionChunk;
        if (head > hi) head = hi;
        unsigned tail = hi / kMotionChunk * kMotionChunk;
        if (tail < head) tail = head;
        T m = T(0.0);
        for (unsigned j = lo + lane; j < head; j += 64u) m = max_rn(m, length[j]);
        for (unsigned c = head / kMotionChunk + lane; c < tail / kMotionChunk; c += 64u) m = max_rn(m, chunk[c]);
        for (unsigned j = tail + lane; j < hi; j += 64u) m = max_rn(m, length[j]);
        m = wave_max_real(m);
        if (lane == k) motion[i] = { T(0.0), T(0.0), T(0.0), m * (T(1.0) + T(kRefitK) * eps<T>()) };
    }
}

}  // namespace rt
