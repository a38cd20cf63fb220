// rt_impacts.hpp -- rt_scene_impacts / rt_scene_impacts_device: every pair of spheres of the scene that comes into contact during one step,
// and when.  The continuous collision step of a particle caller: rt_contacts.hpp's self-join with rt_sweep.hpp's cast as
// its metric, both spheres moving.
//
// For two item slots i < j with stream records {c_i, rr_i} and {c_j, rr_j} and displacements d_i, d_j (sphere k is at c_k + t d_k for t in
// [0, 1]), in REAL, every operation rounded once, no FMA contraction, every root correctly rounded (sqrt_rn_lean), every dot product dot()'s:
//     c' = c S    r' = r S           d' = d S    E' = E S       S: the call's power of two, below; r: the record's radius, below
//     v = c_j' - c_i'          w = d_i' - d_j'                   the lower slot is the query
//     R = (r_j' + E') + r_i'                  RR = R * R         E = 0 for an item
//     a = dot(w, w)    b = dot(v, w)    c = dot(v, v) - RR       disc = b*b - a*c
//     t = +inf                     if !(rr_i > 0 && rr_j > 0)
//       = 0                        else if !(c > 0)              in contact at the start
//       = +inf                     else if !(b > 0) or disc < 0  not approaching (w = 0 too), or passing by
//       = c / (b + sqrt(disc))     otherwise                     the smaller root of a t^2 - 2 b t + c = 0, without a division by a
// (i, j) is an IMPACT when t <= 1.
//
// The stream's rr = r * r says whether a record is alive; the radius itself is the scene's own r -- the item's in the scene's item array, a
// bound's as it was given or refit (a static scene's go up once with the first call, k_impact_bound_radii gathers a dynamic scene's per
// call).  sqrt(r * r) is r wherever r * r is a normal number, and a few bits of it where it is not (f32: r below 2^-63).
//
// a, b and c are of the second degree in a length and disc of the fourth: at the scene's own scale b*b and a*c leave the normal range of f32
// once lengths pass 2^30 or fall below 2^-30.  t has no dimension, so every input is first multiplied by S = 2^-e, exactly: M is the largest of
// |C.x|, |C.y|, |C.z|, r over the stream's nodes with RRn > 0 -- items and bounds -- and of |d.x|, |d.y|, |d.z| over its live items
// (a dead record has no positive rr and contributes nothing, as for D), M = f 2^e with 0.5 <= f < 1, e held to [MIN_EXP + 1, MAX_EXP - 2] so
// that S is normal, S = 1 for M = 0.  Every scaled magnitude is below 1, and lengths down to 2^-31 M keep their fourth powers normal.  The
// products with S are exact wherever the result is normal, so S changes no bit of t there.  k_impact_motion_items folds M into one word
// with an atomic maximum on its bits (M >= 0: the order of the bits is the order of the values; max is exact, so the word is the same
// every time); k_impact_motion_bounds and the walk read S from it.
//
// A bound {C, RRn} that encloses its items at the start of the step encloses them during all of it once its radius grows by the largest
// displacement below it.  The MOTION TABLE, one record {e.x, e.y, e.z, E} per stream node, carries that: an ITEM node of slot j holds
// {d_j, 0}, a BOUND node {0, 0, 0, D} with D = max m_j * (1 + kRefitK eps) over the live items of its subtree -- the stream range (node,
// skip) -- and m_j the length of d_j by the refit's rule (rt_dynamic.hpp): sqrt(s) where s = dot(d_j, d_j) >= refit_tiny, else |dx| + |dy|
// + |dz|; 0 for a record without a positive rr.  The table holds the SCALED values and, in its fourth field, the node's whole
// radius term r' + E': {d_j S, r_j S} and {0, 0, 0, r S + D S} (the lengths and D come from the caller's d, then one product), so the walk
// takes no root.  The walk then applies ONE formula to every node, w = d_i' - e' and R = (r_j' + E') + r_i' as stored: for an item
// that is the definition bit for bit, for a bound the cast of the query (its own motion stays in w) against a standing sphere of radius
// r + D.  A lane culls a bound's subtree when !(t <= 1).
//
// The table is made per call: k_impact_motion_items writes every node's record ({d, r} or {0, 0, 0, r}, unscaled: M is not known yet) and length m (0 for a
// bound) and folds the lengths of kMotionChunk consecutive nodes into one maximum, and the magnitudes into M; k_impact_motion_bounds gives a
// wave 64 consecutive nodes, scales the item records among them, and for each bound among them the wave folds the range (node, skip):
// single lengths up to the first chunk boundary, whole chunks, single lengths behind the last boundary.  max is exact, so the split cannot
// show in the bytes.
//
// The walk is built as k_contact_pairs's is (rt_contacts.hpp) from rt_walk.hpp's pieces -- swept_time is the formula above, bound_step_min
// the wave's step: lane t carries item slot t and walks only the stream behind its own node, the node's motion record arrives through the
// scalar cache next to its stream record, and the wave continues at the smallest resume when nobody enters.  Count pass,
// rt_contacts.hpp's scan, fill pass: the list is sorted by (i, j) and the same bytes every time.
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
    const T *magnitude;             // M of this call (impact_scale)
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

// S of the definition above from M >= 0: 2^-e for M = f 2^e, 0.5 <= f < 1, on the exponent field alone (a denormal M counts as the smallest
// normal number, and the field is held to 252 / 2044 so that S stays normal); 1 for M = 0.
__device__ __forceinline__ float impact_scale(float m)
{
    const unsigned e = __float_as_uint(m) >> 23;
    const unsigned held = e < 1u ? 1u : (e > 252u ? 252u : e);
    return m > 0.0f ? __uint_as_float((253u - held) << 23) : 1.0f;
}
__device__ __forceinline__ double impact_scale(double m)
{
    const unsigned long long e = (unsigned long long)__double_as_longlong(m) >> 52;
    const unsigned long long held = e < 1ull ? 1ull : (e > 2044ull ? 2044ull : e);
    return m > 0.0 ? __longlong_as_double((long long)((2045ull - held) << 52)) : 1.0;
}

template <typename T, bool COUNT, bool FILL>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(8))) void k_impact_pairs(ImpactArgs<T> a)
{
    static_assert(!(COUNT && FILL), "the counters are the first pass's");
    const unsigned t = lane_query(false, nullptr, a.n_items);
    const bool in = t < a.n_items;
    const T S = impact_scale(*a.magnitude);      // (wave-uniform)
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
            p = { me->a0 * S, me->a1 * S, me->a2 * S };
            d = { mine.x, mine.y, mine.z };                          // (the table's: scaled)
            q = mine.E;                                              // (r_i S)
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
            V3<T> v, w;
            const T tm = swept_time(nd, mo, S, p, d, q, v, w);       // the definition above, one formula for both kinds of node
            const bool within = tm <= T(1.0);
            unsigned ni;
            if (nd.is_bound()) {                                     // BOUND  inflated by the largest displacement below it
                const bool cull = active && !within;
                ni = bound_step_min<COUNT>(active, cull, nd, i, resume, c_bounds);
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
    if constexpr (COUNT)
        flush_counters(a.counters, wave_sum(live ? 1u : 0u), wave_sum((live && found > 0u) ? 1u : 0u), wave_sum(c_items), wave_sum(c_bounds));
}

// ---- the motion table ----

template <typename T> __device__ __forceinline__ T wave_max_real(T v)
{
    for (int off = 32; off > 0; off >>= 1) v = max_rn(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ void atomic_max_bits(float *at, float v) { atomicMax(reinterpret_cast<unsigned *>(at), __float_as_uint(v)); }
__device__ __forceinline__ void atomic_max_bits(double *at, double v)
{
    atomicMax(reinterpret_cast<unsigned long long *>(at), (unsigned long long)__double_as_longlong(v));
}

// A dynamic scene's bound radii, per call: radius[node of bound b] = the current bound's r.
template <typename T>
__global__ __launch_bounds__(256) void k_impact_bound_radii(const Item<T> *__restrict__ bounds, const uint32_t *__restrict__ bound_node, unsigned n_bounds, unsigned n_nodes,
                                                            T *__restrict__ radius)
{
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_bounds) return;
    const uint32_t node = bound_node[b];
    if (node < n_nodes) radius[node] = bounds[b].r;                  // (kNoNode: a group without items has no node)
}

// Thread i looks at node i: an ITEM node of slot j takes {d_j, r_j} (k_impact_motion_bounds scales it) and the length m_j (radius and
// length 0 without a positive rr), a BOUND node {0, 0, 0, r} and the length 0 (k_impact_motion_bounds finishes its record).  Block b leaves the largest length of its kMotionChunk
// nodes in chunk[b] and folds the largest magnitude of its nodes into *magnitude, which the caller has set to 0.  disp == NULL (rt_swept.hpp:
// the scene stands still) is a displacement of 0 for every slot.
template <typename T>
__global__ __launch_bounds__(kMotionChunk) void k_impact_motion_items(const Node<T> *__restrict__ stream, const Item<T> *__restrict__ items,
                                                                      const T *__restrict__ bound_radius, const T *__restrict__ disp, unsigned n_nodes, unsigned n_items,
                                                                      Motion<T> *__restrict__ motion, T *__restrict__ length, T *__restrict__ chunk,
                                                                      T *__restrict__ magnitude)
{
    __shared__ T part[kMotionChunk / 64], part_g[kMotionChunk / 64];
    const unsigned i = blockIdx.x * kMotionChunk + threadIdx.x;
    T m = T(0.0), g = T(0.0);
    if (i < n_nodes) {
        const uint32_t word = stream[i].item;
        const uint32_t slot = word & kNodeIndexMask;
        const bool alive = (word & kNodeEnd) == 0u && stream[i].a3 > T(0.0);
        const bool item = (word & kNodeItem) != 0u && (word & kNodeEnd) == 0u && slot < n_items;
        T r = T(0.0);
        if (alive) {
            if (item) r = abs_rn(items[slot].r);
            else if ((word & kNodeItem) == 0u && bound_radius) r = abs_rn(bound_radius[i]);
            g = max_rn(max_rn(abs_rn(stream[i].a0), abs_rn(stream[i].a1)), max_rn(abs_rn(stream[i].a2), r));
        }
        if (item) {
            const T dx = disp ? disp[3 * (size_t)slot] : T(0.0), dy = disp ? disp[3 * (size_t)slot + 1] : T(0.0), dz = disp ? disp[3 * (size_t)slot + 2] : T(0.0);
            motion[i] = { dx, dy, dz, r };
            if (alive) {
                const T s = (dx * dx + dy * dy) + dz * dz;
                m = s >= refit_tiny<T>() ? sqrt_rn_lean(s) : (abs_rn(dx) + abs_rn(dy)) + abs_rn(dz);
                g = max_rn(g, max_rn(max_rn(abs_rn(dx), abs_rn(dy)), abs_rn(dz)));
            }
        } else {
            motion[i] = { T(0.0), T(0.0), T(0.0), r };                   // (a BOUND's record is finished by k_impact_motion_bounds; no node is left undefined)
        }
        length[i] = m;
    }
    m = wave_max_real(m);
    g = wave_max_real(g);
    if ((threadIdx.x & 63u) == 0u) { part[threadIdx.x >> 6] = m; part_g[threadIdx.x >> 6] = g; }
    __syncthreads();
    if (threadIdx.x == 0) {
        T all = part[0], all_g = part_g[0];
        for (unsigned k = 1; k < kMotionChunk / 64; ++k) { all = max_rn(all, part[k]); all_g = max_rn(all_g, part_g[k]); }
        chunk[blockIdx.x] = all;
        if (all_g > T(0.0)) atomic_max_bits(magnitude, all_g);
    }
}

// One wave per 64 consecutive nodes; every other node's record is scaled by S, and for every BOUND among them the whole wave folds the
// lengths of the stream range (node, skip).
template <typename T>
__global__ __launch_bounds__(256) void k_impact_motion_bounds(const Node<T> *__restrict__ stream, unsigned n_nodes, const T *__restrict__ length,
                                                              const T *__restrict__ chunk, const T *__restrict__ magnitude, Motion<T> *__restrict__ motion)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned base = (blockIdx.x * 256u + threadIdx.x) - lane;
    if (base >= n_nodes) return;                                     // (wave-uniform)
    const T S = impact_scale(*magnitude);
    const unsigned i = base + lane;
    bool bound = false;
    unsigned skip = 0;
    if (i < n_nodes) {
        const Node<T> *const nd = stream + i;
        bound = (nd->item & (kNodeItem | kNodeEnd)) == 0u;
        skip = nd->skip_off / (unsigned)sizeof(Node<T>);
        if (!bound) {
            const Motion<T> own = motion[i];
            motion[i] = { own.x * S, own.y * S, own.z * S, own.E * S };
        }
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
        if (lane == k) motion[i] = { T(0.0), T(0.0), T(0.0), motion[i].E * S + (m * (T(1.0) + T(kRefitK) * eps<T>())) * S };
    }
}

}  // namespace rt
