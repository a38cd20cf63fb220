// rt_contacts.hpp -- rt_scene_contacts / rt_scene_contacts_device: every pair of spheres of the scene that is closer than a margin
// (DESIGN.md 4.16).  The broad phase of a collision step, the neighbour list of a relaxation step: a self-join over the scene's own stream.
//
// For two item slots i < j with stream records {c_i, rr_i} and {c_j, rr_j} (rr = the radius squared, rounded once: per_origin_terms,
// rt_skip.hpp), in REAL, every operation rounded once, no FMA contraction, every root correctly rounded (sqrt_rn_lean):
//     v   = c_j - c_i
//     vv  = (v.x*v.x + v.y*v.y) + v.z*v.z                                     dot()'s order
//     gap = (rr_i > 0 && rr_j > 0) ? (sqrt(vv) - sqrt(rr_j)) - sqrt(rr_i) : +inf
// rt_near.hpp's gap of record j from the point c_i, minus the query sphere's own radius.  The LOWER slot is always the query, so the
// rounding of a pair is defined once.  The pair is a CONTACT when !(gap >= margin).  The dead record of DESIGN.md 4.13 is {0, 0, 0, -inf}:
// a dead item carries no query and, as a record, is at +inf -- never part of a pair; a dead BOUND culls for every query.
//
// The walk is made of rt_walk.hpp's pieces (centre_gap, bound_step_min) with the scene's items as the queries: lane t carries item slot t,
// reads its own record from the stream and walks only the part of the stream BEHIND its own node.  Items appear in the stream in ascending
// slot order, so these are exactly the items j > t: every pair is tested once, from its lower slot.  A lane sleeps while i < resume, and a
// lane whose own bound test culls a subtree sets resume = skip.  The wave starts at the smallest resume of its lanes; when no awake lane
// enters a bound it continues at the smallest resume again -- the skip target, or the first node behind a lane that still sleeps inside
// that subtree.
//
// The list is deterministic and compact without an atomic append: the walk runs twice.  The first pass writes one count per item; an
// exclusive scan turns the counts into offsets; the second pass repeats the walk and writes pair offsets[t] + (rank within t) where that
// lies below the capacity.  The pairs are sorted by (i, j) by construction, and a capacity that is too small gets the exact prefix.
#pragma once
#include "rt_walk.hpp"

namespace rt {

template <typename T> struct ContactArgs {
    const Node<T> *stream;          // plain per-origin stream, END-padded
    const uint32_t *item_node;      // [n_items]: the node of every item slot, or NULL: item t is node t (a scene without bounds)
    uint32_t *counts;               // first pass: [n_items], the pairs item t has as the lower slot
    const uint64_t *offsets;        // FILL: [n_items + 1], the exclusive scan of counts
    int32_t *pairs;                 // FILL: [2 capacity]
    T *gap;                         // FILL: [capacity] or NULL
    Counters *counters;             // COUNT: kCounterStripes slots
    T margin;
    uint32_t n_nodes;               // nodes in front of END
    uint32_t n_items;
    uint32_t capacity;              // FILL: pairs the caller has room for
};

template <typename T, bool COUNT, bool FILL>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_contact_pairs(ContactArgs<T> a)
{
    static_assert(!(COUNT && FILL), "the counters are the first pass's");
    const unsigned t = lane_query(false, nullptr, a.n_items);
    const bool in = t < a.n_items;
    V3<T> p = { T(0.0), T(0.0), T(0.0) };
    T q = T(0.0);
    unsigned resume = kNever;                    // a lane without a live item never wakes
    if (in) {
        const unsigned node = a.item_node ? a.item_node[t] : t;
        const Node<T> *const me = a.stream + (node < a.n_nodes ? node : 0u);
        const T rr = me->a3;
        if (node < a.n_nodes && rr > T(0.0)) {                       // (a slot the stream does not hold has no node: no query)
            p = { me->a0, me->a1, me->a2 };
            q = sqrt_rn_lean(rr);
            resume = node + 1u;
        }
    }
    const bool live = resume != kNever;
    const T margin = a.margin;
    unsigned long long at = 0;                   // FILL: where item t's pairs start
    if (FILL) at = live ? a.offsets[t] : 0ull;
    unsigned found = 0;
    unsigned c_items = 0, c_bounds = 0;
    const unsigned n = a.n_nodes;
    const unsigned first = wave_min_u32(resume);
    if (first < n) {
        unsigned i = (unsigned)__builtin_amdgcn_readfirstlane((int)first);
        Node<T> nd = a.stream[i];
        for (;;) {
            const bool active = i >= resume;
            const T g = centre_gap(nd, p, q);                        // the gap above: the lane's own radius comes off
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  against the margin
                const bool cull = active && (g >= margin);
                ni = bound_step_min<COUNT>(active, cull, nd, i, resume, c_bounds);
            } else {                                                 // ITEM   a contact of the lane's item with a later one
                const bool hit = active && !(g >= margin);
                if (FILL) {
                    const unsigned long long pos = at + found;
                    if (hit && pos < (unsigned long long)a.capacity) {
                        a.pairs[2 * pos] = (int32_t)t;
                        a.pairs[2 * pos + 1] = (int32_t)nd.index();
                        if (a.gap) a.gap[pos] = g;
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
    if (!FILL && in) a.counts[t] = found;
    if constexpr (COUNT)
        flush_counters(a.counters, wave_sum(live ? 1u : 0u), wave_sum((live && found > 0u) ? 1u : 0u), wave_sum(c_items), wave_sum(c_bounds));
}

// The item-to-node table of a scene that was not created dynamic: thread i looks at node i, an ITEM node writes its index.
template <typename T>
__global__ void k_contact_item_nodes(const Node<T> *__restrict__ stream, unsigned n_nodes, unsigned n_items, uint32_t *__restrict__ item_node)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const uint32_t word = stream[i].item;
    if ((word & kNodeItem) != 0u && (word & kNodeIndexMask) < n_items) item_node[word & kNodeIndexMask] = i;
}

// ---- the exclusive scan of the counts: uint32 counts[n] -> uint64 offsets[n + 1], three kernels ----
//   k_contact_scan_sums     block b adds up its kScanBlock counts                                   -> sums[b]
//   k_contact_scan_spine    ONE block turns sums[] into its own exclusive scan, kScanBlock at a time with a carry; the carry that is left is
//                           the total: offsets[n] (and the caller's copies of it)
//   k_contact_scan_offsets  block b scans its counts again and adds sums[b]                          -> offsets[b kScanBlock ..]
constexpr unsigned kScanBlock = 256;

// Exclusive scan of one value per thread over a block of kScanBlock threads (Hillis-Steele in LDS); *total: the block's sum, in every thread.
__device__ __forceinline__ unsigned long long block_exclusive_scan(unsigned long long v, unsigned long long *lds, unsigned long long *total)
{
    const unsigned tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (unsigned d = 1; d < kScanBlock; d <<= 1) {
        const unsigned long long below = tid >= d ? lds[tid - d] : 0ull;
        __syncthreads();
        lds[tid] += below;
        __syncthreads();
    }
    const unsigned long long incl = lds[tid];
    *total = lds[kScanBlock - 1];
    __syncthreads();                                                 // (the caller may scan again through the same LDS)
    return incl - v;
}

__global__ __launch_bounds__(kScanBlock) void k_contact_scan_sums(const uint32_t *__restrict__ counts, unsigned n, uint64_t *__restrict__ sums)
{
    __shared__ unsigned long long lds[kScanBlock];
    const unsigned i = blockIdx.x * kScanBlock + threadIdx.x;
    unsigned long long total;
    (void)block_exclusive_scan(i < n ? counts[i] : 0u, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanBlock) void k_contact_scan_spine(uint64_t *__restrict__ sums, unsigned n_sums, uint64_t *__restrict__ end, uint64_t *__restrict__ end_out,
                                                                   uint64_t *__restrict__ total_out)
{
    __shared__ unsigned long long lds[kScanBlock];
    unsigned long long carry = 0;
    for (unsigned base = 0; base < n_sums; base += kScanBlock) {     // (base and n_sums are the same in every thread: every thread meets every barrier)
        const unsigned i = base + threadIdx.x;
        unsigned long long total;
        const unsigned long long excl = block_exclusive_scan(i < n_sums ? sums[i] : 0ull, lds, &total);
        if (i < n_sums) sums[i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) {
        *end = carry;
        if (end_out) *end_out = carry;
        if (total_out) *total_out = carry;
    }
}

__global__ __launch_bounds__(kScanBlock) void k_contact_scan_offsets(const uint32_t *__restrict__ counts, unsigned n, const uint64_t *__restrict__ sums,
                                                                     uint64_t *__restrict__ offsets, uint64_t *__restrict__ offsets_out)
{
    __shared__ unsigned long long lds[kScanBlock];
    const unsigned i = blockIdx.x * kScanBlock + threadIdx.x;
    unsigned long long total;
    const unsigned long long excl = block_exclusive_scan(i < n ? counts[i] : 0u, lds, &total);
    if (i < n) {
        const unsigned long long o = sums[blockIdx.x] + excl;
        offsets[i] = o;
        if (offsets_out) offsets_out[i] = o;
    }
}

}  // namespace rt
