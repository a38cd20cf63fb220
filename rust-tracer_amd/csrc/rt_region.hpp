// rt_region.hpp -- rt_overlap_regions / rt_overlap_regions_device: every sphere of the scene that reaches into each convex REGION of a batch,
// a region being six planes.  A camera's frustum, a screen rectangle's pyramid, a tilted trigger volume, an oriented box.
//
// Region g is planes[24g .. 24g+24] = six {n.x, n.y, n.z, d}; the OUTSIDE of a plane is where n.c + d > 0.  For a stream record {c, rr} (rr =
// the radius squared, rounded once: per_origin_terms, rt_skip.hpp), in REAL, every operation rounded once, no FMA contraction, the root
// correctly rounded (sqrt_rn_lean):
//     s_k = ((n_k.x*c.x + n_k.y*c.y) + n_k.z*c.z) + d_k                       dot()'s order, then + d
//     m   = -inf;  for k = 0..5:  m = s_k > m ? s_k : m                       a comparison, not fmax
//     gap = rr > 0 ? m - sqrt(rr) : +inf
// With unit normals m is the largest signed plane distance of the centre, never above its true distance from the region: the list is a
// SUPERSET of the exact touch list, larger only for spheres outside near an edge or a corner (the usual sphere / frustum test).  An item is
// LISTED when !(gap >= margin), a bound CULLS when gap >= margin (a bound without a positive rr: always).  An absent plane is {0, 0, 0, -inf}:
// s = -inf for every finite centre.  A region carries a query exactly when none of its 24 reals is NaN; any other region makes no test and
// lists nothing.  The dead record of DESIGN.md 4.13 is {0, 0, 0, -inf}: a dead item is at +inf -- never listed -- and a dead BOUND culls.
//
// The walk is the INVERSE of the other query kernels': there a lane carries a query and the wave's node index is uniform (records through
// the scalar cache); here a wave carries ONE region -- its planes are the same in every lane, loaded through the scalar cache into scalar
// registers -- and each lane carries a SECTION of the node stream, with node records as per-lane loads.  A handful of huge regions then
// fills the device where one region per lane would leave one wave walking while the rest idles (DESIGN.md 4.22's `large` rows).
//   Region g is cut into J = a.sections sections; section j is the nodes [floor(j N / J), floor((j + 1) N / J)), N = n_nodes.  Wave w of
// the grid carries sections 64 (w % W) .. + 63 of region w / W, W = ceil(J / 64); lanes past J and empty sections idle.
//   A lane with section [s, e) walks ONE loop from node 0.  While i < s it DESCENDS: a BOUND with skip > s is an ancestor of s -- it is
// tested and counted; culling sets i = skip, which lies behind s and so ends the descent -- and any other node is stepped over (i = skip)
// untested.  A descent that no ancestor ends arrives at exactly i == s.  From there to e it is the one-lane walk: a BOUND culls to skip or
// enters i + 1, an ITEM is tested and i advances.  Every node of [s, e) has its ancestors inside the section or among the ancestors of s,
// so the sections' lists, in section order, are the one-lane walk's list from node 0 (DESIGN.md 4.23 has the argument).  i only grows and
// is compared with e <= n_nodes before every fetch: the walk ends whatever the planes' bits are.
//
// The list is rt_contacts.hpp's, in rt_overlap.hpp's workspace, over n J counts: the first pass writes counts[g J + j]; the exclusive scan
// turns them into offsets; the second pass repeats the walk of every section that counted something and writes entry offsets[g J + j] + rank
// where that lies below the capacity.  Sections are in stream order and the stream's items in slot order: the entries are sorted by
// (g, item slot) by construction, the same bytes for every J.  k_region_rows then gives the caller offsets_out[g] = offsets[g J].
//
// region_gap (rt_walk.hpp) is called, not restated: the six instantiations hold no scratch (tests/test_region_host.py reads their registers).
#pragma once
#include "rt_contacts.hpp"

namespace rt {

template <typename T> struct RegionArgs {
    const Node<T> *stream;          // plain per-origin stream, END-padded
    const T *planes;                // [24 n]: six {n.x, n.y, n.z, d} per region
    uint32_t *counts;               // [n J]: written by the first pass, read by FILL
    const uint64_t *offsets;        // FILL: [n J + 1], the exclusive scan of counts
    int32_t *items;                 // FILL: [capacity]
    T *gap;                         // FILL: [capacity] or NULL
    Counters *counters;             // COUNT: kCounterStripes slots
    T margin;
    uint32_t n_nodes;               // nodes in front of END
    uint32_t n;                     // regions
    uint32_t sections;              // J: 1 .. n_nodes, n J <= 2^26
    uint32_t capacity;              // FILL: entries the caller has room for
};

template <typename T, bool COUNT, bool FILL>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_overlap_regions(RegionArgs<T> a)
{
    static_assert(!(COUNT && FILL), "the counters are the first pass's");
    const unsigned J = a.sections, N = a.n_nodes;
    const unsigned per = (J + 63u) / 64u;                                     // waves per region
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * kBlockThreads + threadIdx.x) / 64u));
    const unsigned g = wave / per, part = wave % per;                         // wave-uniform
    if (g >= a.n) return;                                                     // (the grid's last block may hold waves past the last region)
    const unsigned j = part * 64u + (threadIdx.x & 63u);
    T pl[24];
    bool carried = true;
    const T *const rec = a.planes + 24 * (size_t)g;
#pragma unroll
    for (int k = 0; k < 24; ++k) {
        pl[k] = rec[k];
        carried = carried && (pl[k] == pl[k]);                                // (NaN fails the comparison)
    }
    const size_t slot = (size_t)g * J + j;                                    // < n J <= 2^26 where j < J
    unsigned s = 0, e = 0;                                                    // an idle lane: the empty section
    unsigned long long at = 0;                                                // FILL: where the section's entries start
    if (j < J && carried) {
        bool walks = true;
        if (FILL) walks = a.counts[slot] != 0u;                               // nothing to write: no walk
        if (walks) {
            s = (unsigned)(((unsigned long long)j * N) / J);
            e = (unsigned)(((unsigned long long)(j + 1u) * N) / J);
            if (FILL) at = a.offsets[slot];
        }
    }
    const T margin = a.margin;
    unsigned found = 0;
    unsigned c_items = 0, c_bounds = 0;
    unsigned i = 0;
    while (i < e) {                                                           // e <= n_nodes: no fetch at or behind END
        const Node<T> nd = a.stream[i];
        const unsigned behind = nd.skip() > i ? nd.skip() : i + 1u;           // (a skip target lies behind its node; i grows whatever it reads)
        const bool bound = nd.is_bound();
        if (i < s && !(bound && behind > s)) { i = behind; continue; }        // the descent steps over what is no ancestor of s
        const T t = region_gap(nd, pl);                                       // the gap above
        if (bound) {                                                          // BOUND  against the margin (an ancestor of s, or inside the section)
            if (COUNT) c_bounds += 1u;
            i = (t >= margin) ? behind : i + 1u;
        } else {                                                              // ITEM   within the margin of the wave's region
            const bool hit = !(t >= margin);
            if (FILL) {
                const unsigned long long pos = at + found;
                if (hit && pos < (unsigned long long)a.capacity) {
                    a.items[pos] = (int32_t)nd.index();
                    if (a.gap) a.gap[pos] = t;
                }
            }
            found += hit ? 1u : 0u;
            if (COUNT) c_items += 1u;
            i += 1u;
        }
    }
    if (!FILL && j < J) a.counts[slot] = found;
    if constexpr (COUNT)                                                      // (hits -- regions with an entry -- are k_region_rows's)
        flush_counters(a.counters, wave_sum((carried && j == 0u) ? 1u : 0u), 0ull, wave_sum(c_items), wave_sum(c_bounds));
}

// The caller's rows from the sections' offsets: thread g gives offsets_out[g] = offsets[g J] (thread n: the total), and, counting, the
// regions with an entry go into `hits`.  offsets: [n J + 1], the scan's; offsets_out: [n + 1] or NULL; counters: or NULL.
__global__ __launch_bounds__(kBlockThreads) void k_region_rows(const uint64_t *__restrict__ offsets, unsigned n, unsigned J, uint64_t *__restrict__ offsets_out,
                                                               Counters *counters)
{
    const unsigned g = blockIdx.x * kBlockThreads + threadIdx.x;
    unsigned long long first = 0, next = 0;
    if (g <= n) first = offsets[(size_t)g * J];
    if (g < n) next = offsets[(size_t)(g + 1u) * J];
    if (offsets_out && g <= n) offsets_out[g] = first;
    if (counters) {                                                           // (the same in every thread: every lane meets the shuffles)
        const unsigned long long hits = wave_sum((g < n && next > first) ? 1u : 0u);
        if ((threadIdx.x & 63u) == 0u && hits) atomicAdd(&(counters + blockIdx.x % kCounterStripes)->hits, hits);
    }
}

}  // namespace rt
