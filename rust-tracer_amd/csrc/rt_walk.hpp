// rt_walk.hpp -- the pieces every query kernel's skip-pointer walk is made of, one copy of each: the lane's query index, the five
// metrics, the wave's BOUND and retiring ITEM steps and the counter flush.  The query headers (rt_query.hpp, rt_multihit.hpp,
// rt_near.hpp, rt_sweep.hpp, rt_contacts.hpp, rt_overlap.hpp, rt_impacts.hpp, rt_swept.hpp, rt_first.hpp, rt_box.hpp, rt_region.hpp) call them;
// each kernel keeps its own visible loop -- what accepts, what a hit does, what a lane carries differ in kind -- and its own header says
// what its metric MEANS.  Here is only how each piece is computed.
//
// The walk all of them share (the generic skip-pointer loop of rt_skip.hpp's render_skip_body over the scene's PLAIN per-origin stream):
// the stream index i is wave-uniform (node records arrive through the scalar cache), a lane is awake while i >= its `resume`, a lane
// whose bound test culls sets resume = skip, and the wave jumps once no awake lane wants to enter.  The index only grows (a skip target
// lies behind its node), so every walk ends whatever bits its queries carry.
//
// Everything is REAL arithmetic in a fixed order, every operation rounded once, no FMA contraction, every root sqrt_rn_lean, every dot
// product dot()'s: the host-side walkers of the tests restate these expressions and compare bit for bit.
//
// A function here is optimised on its own before it is inlined, and the kernels are sensitive to that: where calling a piece made an
// instantiation more than one instruction longer than the same text in place, or cost it a register class, that kernel keeps the
// piece in its own text and its header says so (k_near_spheres: the gap and the BOUND step; k_swept_overlaps: the BOUND step and the
// normal; k_query_rays_ordered and k_multihit_rays_ordered: kernel texts of their own, made of these pieces; the k-slot sorted list of
// multihit and near: in place in both).  tools/compare_kernel_asm.py is the check; NOTES.md Y has the figures.
#pragma once
#include "rt_skip.hpp"

namespace rt {

constexpr unsigned kNone = 0xFFFFFFFFu;          // no item (an item word's index has 30 bits: kNone and every negative slot match no item)

// The query this lane carries: thread j of the grid carries query j, or, `ordered`, query order[j] (rt_order.hpp) -- and
// kNever where j >= n (one comparison in front of the load).  An index >= n carries no query: j itself, kNever, or an order entry >= n.
// `ordered` is a kernel's ORDERED template flag, or `order != NULL` where the order is optional at run time.
__device__ __forceinline__ unsigned lane_query(bool ordered, const uint32_t *order, unsigned n)
{
    unsigned gid = blockIdx.x * kBlockThreads + threadIdx.x;
    if (ordered) gid = gid < n ? order[gid] : kNever;
    return gid;
}

// ---- the metrics ----

// Sphere::distance_from_ray (primitive.rs:55-72) of the record from the ray {o, d}, in the reference's order.
template <typename T>
__device__ __forceinline__ T ray_sphere_t(const Node<T> &nd, V3<T> o, V3<T> d)
{
    const V3<T> v = { nd.a0 - o.x, nd.a1 - o.y, nd.a2 - o.z };
    const T b = dot(v, d);
    const T disc = (b * b - dot(v, v)) + nd.a3;
    T t = inf<T>();
    if (!(disc < T(0.0))) {
        const T s = sqrt_rn_lean(disc);
        const T t2 = b + s;
        if (!(t2 < T(0.0))) {
            const T t1 = b - s;
            t = t1 > T(0.0) ? t1 : t2;
        }
    }
    return t;
}

// The surface gap between the record and the sphere {p, q} (rt_overlap.hpp, rt_contacts.hpp): rt_near.hpp's gap from the point p, minus
// the lane's radius.  +inf for a record without a positive rr (the dead record of DESIGN.md 4.13); the radius comes off a live record's
// gap only, so a dead record stays at +inf for q = +inf too (inf - inf would be NaN, and NaN is below every margin's !(t >= margin)).
// The record's root is the same value in every lane.
template <typename T>
__device__ __forceinline__ T centre_gap(const Node<T> &nd, V3<T> p, T q)
{
    const V3<T> v = { nd.a0 - p.x, nd.a1 - p.y, nd.a2 - p.z };
    const T vv = dot(v, v);
    T t = inf<T>();
    if (nd.a3 > T(0.0)) t = (sqrt_rn_lean(vv) - sqrt_rn_lean(nd.a3)) - q;
    return t;
}

// The gap between the record and the axis-aligned box [lo, hi] (rt_box.hpp): per axis how far the record's centre lies outside the box --
// the larger of lo - c and c - hi, floored at 0 -- the root of the squares' sum, minus the record's radius.  Comparisons, not fmax: a NaN
// excess fails both and ends as 0.  An infinite side gives an excess of -inf, which the floor takes: no step makes a NaN from lo = -inf or
// hi = +inf.  +inf for a record without a positive rr, as centre_gap.
template <typename T>
__device__ __forceinline__ T box_gap(const Node<T> &nd, V3<T> lo, V3<T> hi)
{
    V3<T> e = { lo.x - nd.a0, lo.y - nd.a1, lo.z - nd.a2 };
    const V3<T> f = { nd.a0 - hi.x, nd.a1 - hi.y, nd.a2 - hi.z };
    e = { f.x > e.x ? f.x : e.x, f.y > e.y ? f.y : e.y, f.z > e.z ? f.z : e.z };
    e = { e.x > T(0.0) ? e.x : T(0.0), e.y > T(0.0) ? e.y : T(0.0), e.z > T(0.0) ? e.z : T(0.0) };
    const T dd = dot(e, e);
    T t = inf<T>();
    if (nd.a3 > T(0.0)) t = sqrt_rn_lean(dd) - sqrt_rn_lean(nd.a3);
    return t;
}

// The gap between the record and the convex region of six planes pl[4k .. 4k+4] = {n.x, n.y, n.z, d} (rt_region.hpp): the largest of the
// six signed plane distances n_k . c + d_k -- each in dot()'s order, then + d -- minus the record's radius.  A comparison, not fmax, from
// -inf: an absent plane {0, 0, 0, -inf} gives -inf for every finite centre and never wins.  +inf for a record without a positive rr, as
// centre_gap.  The planes are the same in every lane of a wave (scalar registers); the record is the lane's own.
template <typename T>
__device__ __forceinline__ T region_gap(const Node<T> &nd, const T (&pl)[24])
{
    T m = -inf<T>();
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const T s = dot(V3<T>{ pl[4 * k], pl[4 * k + 1], pl[4 * k + 2] }, V3<T>{ nd.a0, nd.a1, nd.a2 }) + pl[4 * k + 3];
        m = s > m ? s : m;
    }
    T t = inf<T>();
    if (nd.a3 > T(0.0)) t = m - sqrt_rn_lean(nd.a3);
    return t;
}

template <typename T> struct Motion;             // a node's motion record {x, y, z, E}: rt_impacts.hpp, with the table it comes from

// The swept pair in the scaled frame (rt_impacts.hpp, rt_swept.hpp): v from the lane's centre p to the record's, w the lane's
// displacement d against the node's motion record mo, both as the swept time below uses them.
template <typename T>
__device__ __forceinline__ void swept_frame(const Node<T> &nd, const Motion<T> &mo, T S, V3<T> p, V3<T> d, V3<T> &v, V3<T> &w)
{
    v = { nd.a0 * S - p.x, nd.a1 * S - p.y, nd.a2 * S - p.z };
    w = { d.x - mo.x, d.y - mo.y, d.z - mo.z };
}

// The time in [0, 1] at which the lane's moving sphere {p, q, d} (scaled by S) first touches the node (rt_impacts.hpp's definition, one
// formula for both kinds of node): 0 in contact at the start, +inf when not approaching, passing by, or the record is dead.  v and w
// come back for the normal.
template <typename T>
__device__ __forceinline__ T swept_time(const Node<T> &nd, const Motion<T> &mo, T S, V3<T> p, V3<T> d, T q, V3<T> &v, V3<T> &w)
{
    swept_frame(nd, mo, S, p, d, v, w);
    const T R = mo.E + q;                                            // ((r_j' + E') + r_i')
    const T RR = R * R;
    const T qa = dot(w, w), qb = dot(v, w), qc = dot(v, v) - RR;
    const T disc = qb * qb - qa * qc;
    T tm = inf<T>();
    if (nd.a3 > T(0.0)) {
        if (!(qc > T(0.0))) tm = T(0.0);
        else if (qb > T(0.0) && !(disc < T(0.0))) tm = qc / (qb + sqrt_rn_lean(disc));
    }
    return tm;
}

// The contact normal of a swept pair at time t (rt_swept.hpp): the lane's centre minus the touched sphere's, normalized.
template <typename T>
__device__ __forceinline__ V3<T> swept_normal(V3<T> v, V3<T> w, T t)
{
    return normalized(V3<T>{ w.x * t - v.x, w.y * t - v.y, w.z * t - v.z });
}

// ---- the wave's steps: from what the lanes decided at node i to the node the wave looks at next ----

// BOUND, every lane walks from node 0 (query, multihit, near, sweep): a culling lane sleeps until the skip target; nobody enters: the
// wave goes there too (no lane's resume lies inside the subtree).
template <bool COUNT, typename T>
__device__ __forceinline__ unsigned bound_step_skip(bool active, bool cull, const Node<T> &nd, unsigned i, unsigned &resume, unsigned &c_bounds)
{
    if (cull) resume = nd.skip();
    if (COUNT) c_bounds += active ? 1u : 0u;
    return (__ballot(active && !cull) == 0) ? nd.skip() : i + 1;
}

// BOUND, lanes may start anywhere (contacts, overlap, impacts, swept, first): nobody enters: every lane's resume now lies behind i -- the
// skip target, or a sleeping lane's own start inside the subtree -- and the wave continues at the smallest.
template <bool COUNT, typename T>
__device__ __forceinline__ unsigned bound_step_min(bool active, bool cull, const Node<T> &nd, unsigned i, unsigned &resume, unsigned &c_bounds)
{
    if (cull) resume = nd.skip();
    if (COUNT) c_bounds += active ? 1u : 0u;
    return (__ballot(active && !cull) == 0) ? wave_min_u32(resume) : i + 1;
}

// ITEM that may finish lanes (fin: this lane needs nothing more): a wave with a newly retired lane goes straight to the smallest resume
// still wanted (the shadow walk's step, rt_skip.hpp); kNever once every lane has retired.
__device__ __forceinline__ unsigned item_step_retire(bool fin, unsigned i, unsigned &resume)
{
    if (fin) resume = kNever;
    return (__ballot(fin) != 0) ? wave_min_u32(resume == kNever ? kNever : (resume > i ? resume : i + 1)) : i + 1;
}

// ---- the counters ----

// One wave's sums into its block's stripe (rt_kernels.hpp), by the wave's first lane.  What counts as a hit differs per kernel: the
// wave_sum calls stay with the caller.
__device__ __forceinline__ void flush_counters(Counters *counters, unsigned long long prim, unsigned long long hits, unsigned long long its, unsigned long long bds)
{
    if ((threadIdx.x & 63u) == 0u) {
        Counters *const stripe = counters + blockIdx.x % kCounterStripes;
        atomicAdd(&stripe->primary, prim);
        atomicAdd(&stripe->hits, hits);
        atomicAdd(&stripe->sphere_tests, its);
        atomicAdd(&stripe->bound_tests, bds);
    }
}

}  // namespace rt
