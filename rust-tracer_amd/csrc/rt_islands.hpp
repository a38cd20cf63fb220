// rt_islands.hpp -- rt_scene_islands / rt_scene_impact_islands (and their _device entries): the connected groups of the contact graph
// (DESIGN.md 4.21).  What a caller that steps spheres wants straight behind the pair list: which spheres belong together -- what it puts
// to sleep, solves on its own, merges or counts as one floating piece.
//
// E: the pairs rt_scene_contacts lists for a margin (rt_contacts.hpp), or rt_scene_impacts for a step (rt_impacts.hpp).  G: the graph on
// the live item slots -- a slot is live when the walk gives it a query: it has a node in the stream and its rr > 0 -- with the edges E.
//     label[i]  the smallest slot of i's connected component of G; -1 for a slot that is not live; i for a live slot without a contact
//     index[i]  the number of islands whose label is below label[i]: dense, 0 .. n_islands - 1, ascending in the label; -1 where label is
//     size[i]   the slots of i's island; 0 where label is -1
//     n_islands the number of i with label[i] == i
//
// The pairs never exist.  The HOOK kernel is k_contact_pairs's walk (k_impact_pairs's for a step), test for test -- lane t carries slot t
// and walks only behind its own node, bound_step_min -- and where that walk would count or write a pair (t, j) it unites t with j in a
// union-find over parent[n_items] in which the LOWER root always wins:
//     find(x)      follow parent until parent[x] == x
//     unite(a, b)  find both roots; lo < hi: compare-and-swap parent[hi] from hi to lo; where that fails, hi had stopped being a root:
//                  go on from the value the swap returned
// parent[x] <= x always, and a root changes only by a swap from itself.  So a tree only ever grows at its root, the root of a tree is its
// minimum, and when the kernel ends -- every edge united -- the root of every component is the component's minimum, whatever the order
// the lanes united in: the labels are one function of the edge set, the same bytes every time.
//
// Every access to parent in the hook kernel is an agent-scope relaxed atomic.  A load may still see an older parent than another CU has
// swapped in; an older parent is an ancestor all the same (a tree never loses a link), so the climb only takes longer.  NO lane ever
// waits for another lane or wave: a climb goes strictly down (parent[x] < x until the root), and a failed swap returns a smaller value to go
// on from.  No flag, no fence, no spin on a value; the kernel boundary is the only ordering: k_island_labels, a kernel of its own,
// reads the finished forest with plain loads.
//
// The counters are the counting pass's of rt_scene_contacts / rt_scene_impacts for the same arguments: the same walk, so nothing may prune
// it by "already in one island".
#pragma once
#include "rt_impacts.hpp"

namespace rt {

// (the stream, the motion table and the forest are kernel arguments of their own, __restrict__: in this struct the compiler could not
// tell the forest's atomics from the node records, and those would leave the scalar cache -- the pair kernels' fill flavours show it)
template <typename T> struct IslandArgs {
    const T *magnitude;             // MOVING: M of this call (impact_scale)
    const uint32_t *item_node;      // [n_items]: the node of every item slot, or NULL: item t is node t (a scene without bounds)
    Counters *counters;             // COUNT: kCounterStripes slots
    T margin;                       // !MOVING
    uint32_t n_nodes;               // nodes in front of END
    uint32_t n_items;
};

__device__ __forceinline__ unsigned island_parent(const uint32_t *parent, unsigned x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One tree out of a's and b's; -> its root as far as this lane sees it.  a: the lane's own root so far (any ancestor of its slot).  Each
// climb ends where parent[x] == x -- a slot that was a root a moment ago -- and goes strictly down until then (parent[x] < x).  The two
// first loads are in flight together: two dependent trips to memory per edge where nobody interferes, not three.
__device__ __forceinline__ unsigned island_unite(uint32_t *parent, unsigned a, unsigned b)
{
    for (;;) {
        unsigned pa = island_parent(parent, a), pb = island_parent(parent, b);
        while (pa != a) { a = pa; pa = island_parent(parent, a); }
        while (pb != b) { b = pb; pb = island_parent(parent, b); }
        if (a == b) return a;
        const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
        unsigned seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return lo;
        a = lo;                                                      // hi hangs below `seen` < hi now: unite lo with that
        b = seen;
    }
}

// parent[t] = t, and size_root[t] = 0 where the call wants sizes.
__global__ __launch_bounds__(256) void k_island_init(uint32_t *__restrict__ parent, uint32_t *__restrict__ size_root, unsigned n_items)
{
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_items) return;
    parent[t] = t;
    if (size_root) size_root[t] = 0u;
}

// The walk of k_contact_pairs (MOVING: of k_impact_pairs, the motion table made as for it), the ITEM step uniting instead of counting.
template <typename T, bool COUNT, bool MOVING>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_island_hook(IslandArgs<T> a, const Node<T> *__restrict__ stream,
                                                                                                         const Motion<T> *__restrict__ motion, uint32_t *__restrict__ parent)
{
    // stream: plain per-origin stream, END-padded; motion: MOVING, [n_nodes], parallel to the stream; parent: [n_items], parent[t] = t going in
    const unsigned t = lane_query(false, nullptr, a.n_items);
    const bool in = t < a.n_items;
    T S = T(1.0);
    if constexpr (MOVING) S = impact_scale(*a.magnitude);            // (wave-uniform)
    V3<T> p = { T(0.0), T(0.0), T(0.0) }, d = { T(0.0), T(0.0), T(0.0) };
    T q = T(0.0);
    unsigned resume = kNever;                    // a lane without a live item never wakes
    if (in) {
        const unsigned node = a.item_node ? a.item_node[t] : t;
        const unsigned at_node = node < a.n_nodes ? node : 0u;
        const Node<T> *const me = stream + at_node;
        const T rr = me->a3;
        if (node < a.n_nodes && rr > T(0.0)) {                       // (a slot the stream does not hold has no node: no query)
            if constexpr (MOVING) {
                const Motion<T> mine = motion[at_node];
                p = { me->a0 * S, me->a1 * S, me->a2 * S };
                d = { mine.x, mine.y, mine.z };                      // (the table's: scaled)
                q = mine.E;                                          // (r_i S)
            } else {
                p = { me->a0, me->a1, me->a2 };
                q = sqrt_rn_lean(rr);
            }
            resume = node + 1u;
        }
    }
    const bool live = resume != kNever;
    const T margin = a.margin;
    unsigned root = t;                           // the lane's own root so far
    unsigned found = 0;                          // COUNT: the pairs the walk would list for t
    unsigned c_items = 0, c_bounds = 0;
    const unsigned n = a.n_nodes;
    const unsigned first = wave_min_u32(resume);
    if (first < n) {
        unsigned i = (unsigned)__builtin_amdgcn_readfirstlane((int)first);
        Node<T> nd = stream[i];
        Motion<T> mo = {};
        if constexpr (MOVING) mo = motion[i];
        for (;;) {
            const bool active = i >= resume;
            bool apart;                                              // the node is no contact (no impact) of the lane's sphere
            if constexpr (MOVING) {
                V3<T> v, w;
                apart = !(swept_time(nd, mo, S, p, d, q, v, w) <= T(1.0));
            } else {
                apart = centre_gap(nd, p, q) >= margin;
            }
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  as the pair walk's
                ni = bound_step_min<COUNT>(active, active && apart, nd, i, resume, c_bounds);
            } else {                                                 // ITEM   an edge of the lane's item to a later one
                const bool hit = active && !apart;
                const unsigned j = nd.index();
                if (hit && j < a.n_items) root = island_unite(parent, root, j);
                if (COUNT) { found += hit ? 1u : 0u; c_items += active ? 1u : 0u; }
                ni = i + 1;
            }
            if (ni >= n) break;                                      // also kNever: every lane is done
            i = (unsigned)__builtin_amdgcn_readfirstlane((int)ni);
            nd = stream[i];
            if constexpr (MOVING) mo = motion[i];
        }
    }
    if constexpr (COUNT)
        flush_counters(a.counters, wave_sum(live ? 1u : 0u), wave_sum((live && found > 0u) ? 1u : 0u), wave_sum(c_items), wave_sum(c_bounds));
}

// Behind the hook kernel: label[t] = the root of t's tree, -1 for a slot that is not live; counts[t] = 1 for a root -- the scan of
// rt_contacts.hpp then gives offsets[l] = the islands whose label is below l, and n_islands as its total; size_root[l] += 1 per member
// where the call wants sizes (integers: the sum is the same in every order).
template <typename T>
__global__ __launch_bounds__(256) void k_island_labels(const Node<T> *__restrict__ stream, const uint32_t *__restrict__ item_node, const uint32_t *__restrict__ parent,
                                                       unsigned n_nodes, unsigned n_items, int32_t *__restrict__ label, uint32_t *__restrict__ counts,
                                                       uint32_t *__restrict__ size_root)
{
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_items) return;
    const unsigned node = item_node ? item_node[t] : t;
    const bool live = node < n_nodes && stream[node < n_nodes ? node : 0u].a3 > T(0.0);
    unsigned x = t;
    if (live)
        for (unsigned up = parent[x]; up != x; up = parent[x]) x = up;
    label[t] = live ? (int32_t)x : -1;
    counts[t] = (live && x == t) ? 1u : 0u;
    if (size_root) {
        // the lanes of a wave that share the first live lane's label add once, together: in a large island that is most of the wave, and
        // one address takes its additions one by one (integers: the sum is the same however it is split)
        const unsigned long long alive = __ballot(live);
        if (alive != 0ull) {                                             // (wave-uniform)
            const unsigned lead = (unsigned)__builtin_ctzll(alive);
            const unsigned l0 = (unsigned)__shfl((int)x, (int)lead, 64);
            const unsigned long long same = __ballot(live && x == l0);
            if (live && x != l0) atomicAdd(size_root + x, 1u);
            if ((threadIdx.x & 63u) == lead) atomicAdd(size_root + l0, (unsigned)__builtin_popcountll(same));
        }
    }
}

// Behind the scan, where the call wants them: index[t] = offsets[label[t]], size[t] = size_root[label[t]].
__global__ __launch_bounds__(256) void k_island_finish(const int32_t *__restrict__ label, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ size_root,
                                                       unsigned n_items, int32_t *__restrict__ index, uint32_t *__restrict__ size)
{
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_items) return;
    const int32_t l = label[t];
    if (index) index[t] = l >= 0 ? (int32_t)offsets[l] : -1;
    if (size) size[t] = l >= 0 ? size_root[l] : 0u;
}

}  // namespace rt
