// rt_filter_bounds.hpp -- the filtered loops' per-node bounds, ONE statement for the device (rt_skip.hpp: k_build_fstreams and its f64 twin) and
// for the host (rt_tight.hpp: the per-walk records are derived from the values the stream kernels will write for the items).  Plain C++ with
// compiler builtins only; every operation is an IEEE double or float operation that rounds the same way on either side.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RT_BOUNDS_FN __host__ __device__ __forceinline__
#else
#define RT_BOUNDS_FN inline
#endif

namespace rt_bounds {

RT_BOUNDS_FN uint32_t bits_of(float f) { return __builtin_bit_cast(uint32_t, f); }
RT_BOUNDS_FN float float_of(uint32_t u) { return __builtin_bit_cast(float, u); }

RT_BOUNDS_FN float next_above(float f)      // finite f
{
    const uint32_t u = bits_of(f);
    if ((u << 1) == 0u) return float_of(0x00000001u);
    return float_of((u >> 31) ? u - 1u : u + 1u);
}
RT_BOUNDS_FN float next_below(float f)      // finite f
{
    const uint32_t u = bits_of(f);
    if ((u << 1) == 0u) return float_of(0x80000001u);
    return float_of((u >> 31) ? u + 1u : u - 1u);
}

// Outer / inner bound of P2 for a sphere with squared radius rr (as the reference rounds it): DESIGN.md 4.1.  S, eta: FilterConsts::S, ::eta.
RT_BOUNDS_FN void shadow_bounds(double S, double eta, float rr_f, float &r2o, float &r2i)
{
    const double eps = 0x1p-24, rr = rr_f, S2 = S * S, a9 = 9.7 * eps * S;
    if (!(rr < 1e300)) { r2o = r2i = __builtin_huge_valf(); return; }       // END: rr = +inf
    const double so = __builtin_sqrt(rr * (1.0 + 1.01 * eps) + (eta + 12.0 * eps) * S2) + a9;
    const double o = so * so * (1.0 + 2.01 * eps) + 1e-36;
    float of = (float)o;
    if ((double)of < o) of = next_above(of);
    r2o = next_above(of);
    // inner bound, for the test  P2 + k1 (P2 + a^2) <= R2i  (FilterConsts::k1 carries the part that grows with the ray's own distance)
    const double tau = 0x1p-10, es2 = eps * S * eps * S;
    const double c2 = 102.7 * (1.0 + 1.0 / tau) * es2 * (1.0 + eta);
    const double X = (1.0 + eta + 10.2 * eps) * c2 * (1.0 + 6.0 * eps) + 94.1 * es2 * (1.0 + 1.0 / tau);
    const double i = (rr * (1.0 - eps) - X) / ((1.0 + tau) * (1.0 + 2.1 * eps) * (1.0 + eta) * (1.0 + 40.0 * eps)) * (1.0 - 8.0 * eps) - 1e-36;
    r2i = -1.0f;
    if (i > 0.0) {
        float inf_ = (float)i;
        if ((double)inf_ > i) inf_ = next_below(inf_);
        inf_ = next_below(inf_);
        r2i = inf_ > 0.0f ? inf_ : -1.0f;
    }
}

// The primary filter's threshold for a node with the stored terms vv = dot(v, v), rr (both as the reference rounds them): rt_skip.hpp,
// primary_filter_threshold, carries the statement; DESIGN.md 4.1 the derivation.
RT_BOUNDS_FN float primary_threshold(float vv_f, float rr_f)
{
    const double eps = 0x1p-24, vv = vv_f, rr = rr_f;
    // (vv >= 1e-14: |v| >= 1e-7, so that b >= sqrt(60 eps vv) keeps the squares of the BOUND step's root-free decision -- differences of
    // values of b's magnitude -- in the normal range: bound_shortcut_verdict)
    if (!(vv >= 1e-14) || !(vv - rr >= 64.0 * eps * (vv + rr))) return -__builtin_huge_valf();
    const double m0 = vv - rr * (1.0 + 2.0 * eps) - 1e-44;
    const double t = __builtin_sqrt(m0 * (1.0 - 2.0 * eps)) - 8.0 * eps * __builtin_sqrt(vv);
    float tf = (float)t;
    if ((double)tf > t) tf = next_below(tf);
    return next_below(tf);
}

// Rq of an eye sphere X with the stored terms vv = dot(v', v'), rr (both as the reference rounds them): the reference's distance to X is
// d_X >= b' - Rq for every ray on which it is finite, b' = fma(v'z, dz, fma(v'y, dy, v'x dx)) as the filter forms it (NOTES.md "Lean bound
// steps").  ES2 = A S^2 of rt_tight.hpp: E(rr) = ES2 + 2 eps rr bounds the f32 discriminant's error, so disc^ <= rr + E(rr) (b^2 - vv <= 0 up
// to those roundings), s^ = RN(sqrt(disc^)) <= sqrt(rr + E(rr)) (1 + eps); b^ is within 4 eps |v'| of b', and the rounding of b^ - s^ costs
// eps (|b^| + s^) <= eps (1.01 |v'| + s^).  Rounded up twice.  +inf where nothing is known (the lean step then culls nobody).
RT_BOUNDS_FN float lean_radius(float vv_f, float rr_f, double ES2)
{
    const double eps = 0x1p-24, vv = vv_f, rr = rr_f;
    if (!(vv < 1e300) || !(rr < 1e300) || !(ES2 < 1e300)) return __builtin_huge_valf();
    const double q = __builtin_sqrt(rr * (1.0 + 2.0 * eps) + ES2) * (1.0 + 4.0 * eps) + 8.0 * eps * __builtin_sqrt(vv) + 1e-44;
    float qf = (float)q;
    if ((double)qf < q) qf = next_above(qf);
    return qf < __builtin_huge_valf() ? next_above(qf) : qf;
}

// What a BOUND node of the per-walk streams carries instead of the values derived from its sphere (rt_tight.hpp build_walk makes them on the
// host, k_build_fstreams applies them): the primary record takes max(T of its sphere, tp); the shadow record takes the disc whole.
struct WalkOverride {
    float tp;                       // kWalkPrimary: T', the cone that holds every item's cap, about the node's own v
    float w1, w2, cl, r2o, r2i;     // kWalkShadow: the light disc (centre in the plane across the light, front along it, outer / inner bound)
    uint32_t flags;
    float rq;                       // kWalkPrimary: Rq of the eye sphere (lean_radius): a lane with b' - Rq >= hit.distance has nothing to find below
};
constexpr uint32_t kWalkPrimary = 1u, kWalkShadow = 2u;
// FNode::tag of a BOUND of the per-walk primary stream that is decided by b' alone (a4 = Rq instead of rr): neither bit 31 (ITEM / END) nor bit 30 (END)
constexpr uint32_t kTagLeanBound = 0x20000000u;
static_assert(sizeof(WalkOverride) == 32, "one 32-byte record per node, like the streams");

}  // namespace rt_bounds
