// rt_dynamic.hpp -- dynamic scenes (rt_scene_create_dynamic / rt_scene_update*): the topology is fixed when the scene is
// made, the sphere values are replaced at any time and the group bounds are given or REFIT here.
//
// What the general-ray kernels read of a scene is its items and ONE stream of Node<T> records (rt_query.hpp).  An update rewrites the
// value fields {cx, cy, cz, rr} of those records -- per_origin_terms (rt_skip.hpp), the arithmetic k_build_streams and k_items_stream use --
// and leaves the item words, the skip offsets and the END padding as they were created: they are the topology, resident on the device
// (k_dynamic_topology), and never depend on a value the caller passes.
//
// The refit rule (include/rtrace_hip.h states it; rust_tracer_amd.refit_bounds restates it in numpy) is min / max over a group's items
// twice: the box, then the reach around the box's centre.  min and max are exact, so a group may be split any way: the host cuts every
// group into WORK records of at most kRefitChunk consecutive items and a wave takes one record.  A leaf group of five items is one wave;
// the pyramid's top group (21,845 items) is 86 waves in as many workgroups' slots, joined through their partial boxes (second pass: every
// wave of the group folds them again, the same bits in each) and an integer atomic max on the reach's bits (a non-negative float orders
// as its bits do).  Three launches whatever the hierarchy: box, reach, rewrite.
#pragma once
#include "rt_skip.hpp"

namespace rt {

constexpr unsigned kRefitChunk = 256;              // items per work record: four coalesced {cx, cy, cz, r} loads per lane
constexpr unsigned kRefitK = 8;                    // radius = max reach * (1 + kRefitK * EPSILON)   (NOTES.md A: 2.75 would do)
constexpr uint32_t kNoNode = 0xFFFFFFFFu;          // a group without items has no node (build_raw_stream drops it)

// One wave's share of a refit: items [first, first + count) of group `group`, whose records are work[pfirst .. pfirst + pcount).
struct alignas(32) RefitWork { uint32_t group, first, count, pfirst, pcount, pad0, pad1, pad2; };
static_assert(sizeof(RefitWork) == 32, "one aligned scalar-load unit");

// Below this sum of squares the distance is taken as |dx| + |dy| + |dz| (>= the Euclidean one, and no product in it): a square that
// underflows would lose the whole distance (f32 spheres at 1e-30: dx * dx = 0).  MIN_NORMAL / EPSILON^2: at or above it what three
// underflowing products can lose is below 2^-44 of the sum.
template <typename T> __device__ __forceinline__ constexpr T refit_tiny();
template <> __device__ __forceinline__ constexpr float refit_tiny<float>() { return 0x1p-80f; }
template <> __device__ __forceinline__ constexpr double refit_tiny<double>() { return 0x1p-918; }

__device__ __forceinline__ float min_rn(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double min_rn(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ float max_rn(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double max_rn(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ float abs_rn(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ double abs_rn(double a) { return __builtin_fabs(a); }

// reach of one item around `c` (step 4 of the rule), every operation rounded once
template <typename T>
__device__ __forceinline__ T refit_reach(const Item<T> &it, T cx, T cy, T cz)
{
    const T dx = it.cx - cx, dy = it.cy - cy, dz = it.cz - cz;
    const T s = (dx * dx + dy * dy) + dz * dz;
    const T dist = s >= refit_tiny<T>() ? rsqrt_exact(s) : (abs_rn(dx) + abs_rn(dy)) + abs_rn(dz);
    return dist + it.r;
}

// v of the lane CTRL names, `id` where there is none (or the row is not in ROWS): the DPP move of wave_min_u32, for 4- and 8-byte values
template <int CTRL, int ROWS> __device__ __forceinline__ float dpp_from(float v, float id)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(id), __float_as_int(v), CTRL, ROWS, 0xf, false));
}
template <int CTRL, int ROWS> __device__ __forceinline__ double dpp_from(double v, double id)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(id), __double2loint(v), CTRL, ROWS, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(id), __double2hiint(v), CTRL, ROWS, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float lane63(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }
__device__ __forceinline__ double lane63(double v)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

// Minimum (MAX: maximum) over the wave's 64 lanes, wave-uniform: four row shifts and the two row broadcasts, no LDS.
template <bool MAX, typename T>
__device__ __forceinline__ T wave_extreme(T v)
{
    const T id = MAX ? -inf<T>() : inf<T>();
#define RT_DPP_EXT(CTRL, ROWS) { const T o = dpp_from<CTRL, ROWS>(v, id); v = MAX ? max_rn(v, o) : min_rn(v, o); }
    RT_DPP_EXT(0x111, 0xf)     // row_shr:1
    RT_DPP_EXT(0x112, 0xf)     // row_shr:2
    RT_DPP_EXT(0x114, 0xf)     // row_shr:4
    RT_DPP_EXT(0x118, 0xf)     // row_shr:8   -> lane 15 of each row holds the row's
    RT_DPP_EXT(0x142, 0xa)     // row_bcast:15 into rows 1 and 3
    RT_DPP_EXT(0x143, 0xc)     // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's
#undef RT_DPP_EXT
    return lane63(v);
}

template <typename T> struct BitsOf;
template <> struct BitsOf<float> { typedef unsigned type; };
template <> struct BitsOf<double> { typedef unsigned long long type; };
__device__ __forceinline__ unsigned bits_of(float v) { return __float_as_uint(v); }
__device__ __forceinline__ unsigned long long bits_of(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ float real_of(unsigned b) { return __uint_as_float(b); }
__device__ __forceinline__ double real_of(unsigned long long b) { return __longlong_as_double((long long)b); }

template <typename T> struct RefitArgs {
    const Item<T> *src;                    // the new items (the caller's device memory, or the scene's staging)
    const RefitWork *work;
    T *pbox;                               // [6 n_work]: lo.xyz, hi.xyz of every work record
    typename BitsOf<T>::type *reach;       // [n_bounds]: bits of the largest reach so far
    Item<T> *bounds;                       // [n_bounds]: the scene's current bounds
    uint32_t n_work;
};

// the wave's work record, or nothing (the last workgroup's spare waves)
template <typename T>
__device__ __forceinline__ bool refit_work(const RefitArgs<T> &a, RefitWork &k, unsigned &w)
{
    w = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlockThreads / 64) + (threadIdx.x >> 6)));
    if (w >= a.n_work) return false;
    k = a.work[w];
    return true;
}

// Steps 1 and 2: lo / hi of one work record.  The group's first record also clears the group's reach for the pass behind this one.
template <typename T>
__global__ __launch_bounds__(kBlockThreads) void k_refit_box(RefitArgs<T> a)
{
    RefitWork k; unsigned w;
    if (!refit_work(a, k, w)) return;
    const unsigned lane = threadIdx.x & 63u;
    T lo[3] = { inf<T>(), inf<T>(), inf<T>() }, hi[3] = { -inf<T>(), -inf<T>(), -inf<T>() };
    for (unsigned j = lane; j < k.count; j += 64u) {
        const Item<T> it = a.src[k.first + j];
        lo[0] = min_rn(lo[0], it.cx - it.r); lo[1] = min_rn(lo[1], it.cy - it.r); lo[2] = min_rn(lo[2], it.cz - it.r);
        hi[0] = max_rn(hi[0], it.cx + it.r); hi[1] = max_rn(hi[1], it.cy + it.r); hi[2] = max_rn(hi[2], it.cz + it.r);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = wave_extreme<false>(lo[c]); hi[c] = wave_extreme<true>(hi[c]); }
    if (lane == 0u) {
        T *p = a.pbox + 6 * (size_t)w;
        p[0] = lo[0]; p[1] = lo[1]; p[2] = lo[2]; p[3] = hi[0]; p[4] = hi[1]; p[5] = hi[2];
        if (w == k.pfirst) a.reach[k.group] = 0;
    }
}

// Steps 3 and 4: the group's box from its records' boxes, its centre, and the largest reach among this record's items.
template <typename T>
__global__ __launch_bounds__(kBlockThreads) void k_refit_reach(RefitArgs<T> a)
{
    RefitWork k; unsigned w;
    if (!refit_work(a, k, w)) return;
    const unsigned lane = threadIdx.x & 63u;
    T lo[3], hi[3];
    if (k.pcount == 1u) {
        const T *p = a.pbox + 6 * (size_t)w;
        lo[0] = p[0]; lo[1] = p[1]; lo[2] = p[2]; hi[0] = p[3]; hi[1] = p[4]; hi[2] = p[5];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = inf<T>(); hi[c] = -inf<T>(); }
        for (unsigned j = lane; j < k.pcount; j += 64u) {
            const T *p = a.pbox + 6 * (size_t)(k.pfirst + j);
#pragma unroll
            for (int c = 0; c < 3; ++c) { lo[c] = min_rn(lo[c], p[c]); hi[c] = max_rn(hi[c], p[3 + c]); }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = wave_extreme<false>(lo[c]); hi[c] = wave_extreme<true>(hi[c]); }
    }
    const T cx = (lo[0] + hi[0]) * T(0.5), cy = (lo[1] + hi[1]) * T(0.5), cz = (lo[2] + hi[2]) * T(0.5);
    T reach = T(0);                                                  // (every reach is >= its radius > 0)
    for (unsigned j = lane; j < k.count; j += 64u) reach = max_rn(reach, refit_reach(a.src[k.first + j], cx, cy, cz));
    reach = wave_extreme<true>(reach);
    if (lane == 0u) {
        atomicMax(a.reach + k.group, bits_of(reach));
        if (w == k.pfirst) { Item<T> *b = a.bounds + k.group; b->cx = cx; b->cy = cy; b->cz = cz; }
    }
}

// The value fields of a stream record as one aligned store.
template <typename T> struct alignas(sizeof(T) * 4) NodeTerms { T a0, a1, a2, a3; };

template <typename T> struct RewriteArgs {
    const Item<T> *src_items;              // the new items
    const Item<T> *src_bounds;             // the caller's bounds, or NULL: refit (centre in `bounds`, reach bits in `reach`)
    Item<T> *items;                        // the scene's items
    Item<T> *bounds;                       // the scene's current bounds
    const typename BitsOf<T>::type *reach;
    Node<T> *stream;                       // the stream the general-ray kernels walk
    const uint32_t *item_node;             // node of every item (NULL: item i is node i, a scene without bounds)
    const uint32_t *bound_node;            // node of every bound, kNoNode for a group without items
    uint32_t n_items, n_bounds;
};

template <typename T>
__device__ __forceinline__ void rewrite_node(Node<T> *stream, uint32_t node, T cx, T cy, T cz, T r)
{
    Node<T> rec;
    per_origin_terms(rec, cx, cy, cz, r);
    *reinterpret_cast<NodeTerms<T> *>(stream + node) = NodeTerms<T>{ rec.a0, rec.a1, rec.a2, rec.a3 };
}

// Step 5 and the rewrite: one thread per node -- the items first, then the bounds.  Item words and skip offsets stay as created.
template <typename T>
__global__ __launch_bounds__(kBlockThreads) void k_dynamic_rewrite(RewriteArgs<T> a)
{
    const unsigned t = blockIdx.x * kBlockThreads + threadIdx.x;
    if (t < a.n_items) {
        const Item<T> it = a.src_items[t];
        a.items[t] = it;
        rewrite_node(a.stream, a.item_node ? a.item_node[t] : t, it.cx, it.cy, it.cz, it.r);
        return;
    }
    const unsigned b = t - a.n_items;
    if (b >= a.n_bounds) return;
    const uint32_t node = a.bound_node[b];
    Item<T> bd;
    if (a.src_bounds) bd = a.src_bounds[b];
    else {
        if (node == kNoNode) return;                                 // a group without items keeps the bound it was given
        bd = a.bounds[b];
        bd.r = real_of(a.reach[b]) * (T(1.0) + T(kRefitK) * eps<T>());
    }
    a.bounds[b] = bd;
    if (node != kNoNode) rewrite_node(a.stream, node, bd.cx, bd.cy, bd.cz, bd.r);
}

// ---- live and dead slots (rt_scene_update_live*, rt_scene_rebuild_n*) ----
// The siblings of the three kernels above for a scene whose slots are LIVE or DEAD: the same launches over the same work records, a lane
// leaves its dead items out.  Liveness is one byte per slot (nonzero = live), or -- PREFIX, what a rebuild of n spheres leaves -- the
// predicate slot < n_live with no byte read.  A work record without a live item keeps the identity box and adds nothing to the reach, so
// a group is dead exactly when its reach bits are still 0 behind the reach pass (a live reach is at least a radius, > 0): the rewrite
// gives such a group, and every dead item, the DEAD RECORD -- centre 0 and rr = -inf, disc = (b*b - vv) + rr = -inf for every ray of the
// domain: an ITEM that is never hit, a BOUND that culls for every ray; the mirror image of per_origin_end's +inf.
template <typename T> struct LiveRefitArgs {
    RefitArgs<T> r;
    const uint8_t *live;                   // [n_items].  PREFIX: not read
    uint32_t n_live;                       // PREFIX: slots [0, n_live) are live
};

template <bool PREFIX>
__device__ __forceinline__ bool slot_live(const uint8_t *live, uint32_t n_live, uint32_t slot)
{
    if (PREFIX) return slot < n_live;
    return live[slot] != 0;                // (a wave's 64 lanes read 64 consecutive bytes: one request)
}

template <typename T, bool PREFIX>
__global__ __launch_bounds__(kBlockThreads) void k_refit_box_live(LiveRefitArgs<T> la)
{
    const RefitArgs<T> &a = la.r;
    RefitWork k; unsigned w;
    if (!refit_work(a, k, w)) return;
    const unsigned lane = threadIdx.x & 63u;
    T lo[3] = { inf<T>(), inf<T>(), inf<T>() }, hi[3] = { -inf<T>(), -inf<T>(), -inf<T>() };
    for (unsigned j = lane; j < k.count; j += 64u) {
        if (!slot_live<PREFIX>(la.live, la.n_live, k.first + j)) continue;
        const Item<T> it = a.src[k.first + j];
        lo[0] = min_rn(lo[0], it.cx - it.r); lo[1] = min_rn(lo[1], it.cy - it.r); lo[2] = min_rn(lo[2], it.cz - it.r);
        hi[0] = max_rn(hi[0], it.cx + it.r); hi[1] = max_rn(hi[1], it.cy + it.r); hi[2] = max_rn(hi[2], it.cz + it.r);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = wave_extreme<false>(lo[c]); hi[c] = wave_extreme<true>(hi[c]); }
    if (lane == 0u) {
        T *p = a.pbox + 6 * (size_t)w;
        p[0] = lo[0]; p[1] = lo[1]; p[2] = lo[2]; p[3] = hi[0]; p[4] = hi[1]; p[5] = hi[2];
        if (w == k.pfirst) a.reach[k.group] = 0;
    }
}

template <typename T, bool PREFIX>
__global__ __launch_bounds__(kBlockThreads) void k_refit_reach_live(LiveRefitArgs<T> la)
{
    const RefitArgs<T> &a = la.r;
    RefitWork k; unsigned w;
    if (!refit_work(a, k, w)) return;
    const unsigned lane = threadIdx.x & 63u;
    T lo[3], hi[3];
    if (k.pcount == 1u) {
        const T *p = a.pbox + 6 * (size_t)w;
        lo[0] = p[0]; lo[1] = p[1]; lo[2] = p[2]; hi[0] = p[3]; hi[1] = p[4]; hi[2] = p[5];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = inf<T>(); hi[c] = -inf<T>(); }
        for (unsigned j = lane; j < k.pcount; j += 64u) {
            const T *p = a.pbox + 6 * (size_t)(k.pfirst + j);
#pragma unroll
            for (int c = 0; c < 3; ++c) { lo[c] = min_rn(lo[c], p[c]); hi[c] = max_rn(hi[c], p[3 + c]); }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = wave_extreme<false>(lo[c]); hi[c] = wave_extreme<true>(hi[c]); }
    }
    // a group without a live item still has the identity box, whose centre would be (+inf + -inf) * 0.5 = NaN: it gets centre 0, nobody
    // takes a reach around it, and the rewrite puts the dead record in its place
    // (x alone decides: a live item puts finite values on all three axes, so either every axis is still the identity or none is)
    const bool any = lo[0] <= hi[0];
    const T cx = any ? (lo[0] + hi[0]) * T(0.5) : T(0), cy = any ? (lo[1] + hi[1]) * T(0.5) : T(0), cz = any ? (lo[2] + hi[2]) * T(0.5) : T(0);
    T reach = T(0);
    for (unsigned j = lane; j < k.count; j += 64u)
        if (slot_live<PREFIX>(la.live, la.n_live, k.first + j)) reach = max_rn(reach, refit_reach(a.src[k.first + j], cx, cy, cz));
    reach = wave_extreme<true>(reach);
    if (lane == 0u) {
        atomicMax(a.reach + k.group, bits_of(reach));
        if (w == k.pfirst) { Item<T> *b = a.bounds + k.group; b->cx = cx; b->cy = cy; b->cz = cz; }
    }
}

template <typename T> struct LiveRewriteArgs {
    RewriteArgs<T> r;
    const uint8_t *live;                   // as LiveRefitArgs
    uint8_t *live_out;                     // [n_items]: the scene's resident liveness, 0 / 1 (rt_scene_live)
    uint32_t n_live;
};

template <typename T>
__device__ __forceinline__ void rewrite_dead(Node<T> *stream, uint32_t node)
{
    *reinterpret_cast<NodeTerms<T> *>(stream + node) = NodeTerms<T>{ T(0), T(0), T(0), -inf<T>() };
}

// The rewrite with dead slots: a dead item's values are not read (its slot of the scene's items is cleared), a refit group that no live
// item reached reports {0, 0, 0, 0}.  The caller's bounds are written as given.  PREFIX with n_live == 0: the refit did not run, every
// group is dead.
template <typename T, bool PREFIX>
__global__ __launch_bounds__(kBlockThreads) void k_dynamic_rewrite_live(LiveRewriteArgs<T> la)
{
    const RewriteArgs<T> &a = la.r;
    const unsigned t = blockIdx.x * kBlockThreads + threadIdx.x;
    if (t < a.n_items) {
        const bool live = slot_live<PREFIX>(la.live, la.n_live, t);
        const uint32_t node = a.item_node ? a.item_node[t] : t;
        la.live_out[t] = live ? 1 : 0;
        if (live) {
            const Item<T> it = a.src_items[t];
            a.items[t] = it;
            rewrite_node(a.stream, node, it.cx, it.cy, it.cz, it.r);
        } else {
            a.items[t] = Item<T>{ T(0), T(0), T(0), T(0) };
            rewrite_dead(a.stream, node);
        }
        return;
    }
    const unsigned b = t - a.n_items;
    if (b >= a.n_bounds) return;
    const uint32_t node = a.bound_node[b];
    Item<T> bd;
    bool dead = false;
    if (a.src_bounds) bd = a.src_bounds[b];
    else {
        if (node == kNoNode) return;                                 // a group without items keeps the bound it was given
        dead = a.reach[b] == 0 || (PREFIX && la.n_live == 0u);
        bd = a.bounds[b];
        bd.r = real_of(a.reach[b]) * (T(1.0) + T(kRefitK) * eps<T>());
        if (dead) bd = Item<T>{ T(0), T(0), T(0), T(0) };
    }
    a.bounds[b] = bd;
    if (node == kNoNode) return;
    if (dead) rewrite_dead(a.stream, node);
    else rewrite_node(a.stream, node, bd.cx, bd.cy, bd.cz, bd.r);
}

// The resident topology of a dynamic scene's stream: item word and skip offset of every node, the END padding whole.  The value fields
// are k_dynamic_rewrite's, which rt_scene_create_dynamic runs behind this.
template <typename T>
__global__ __launch_bounds__(kBlockThreads) void k_dynamic_topology(const uint2 *__restrict__ topo, unsigned n, Node<T> *__restrict__ stream)
{
    const unsigned i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n + kNodePad) return;
    Node<T> s;
    if (i >= n) per_origin_end(s, n);
    else {
        per_origin_terms(s, T(0), T(0), T(0), T(0));
        s.item = topo[i].x;
        s.skip_off = topo[i].y;
    }
    stream[i] = s;
}

}  // namespace rt
