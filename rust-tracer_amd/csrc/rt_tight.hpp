// rt_tight.hpp -- tight bounding spheres for the filtered f32 walks (host only, plain C++: rt_capi_scene.hpp and tools/step_census.cpp share it).
//
// A BOUND node of the skip-pointer stream (rt_skip.hpp) carries the sphere the scene was given.  The walks only need a volume that encloses
// the subtree's items, so a node may carry a smaller sphere B' instead, as long as no decision that reaches the picture changes.  build()
// computes B' bottom-up (an enclosing ball of the node's direct items and its child groups' balls, Badoiu-Clarkson steps in double) and keeps
// it only where rules (a) - (d) below hold, checked in double against every item of the subtree.  NOTES.md ("Tight bounds") derives the
// inflation; in short, with eps = 2^-24, eta >= | |d|^2 - 1 | for every ray direction d, S >= |centre - origin| for every node and origin:
//   the f32 discriminant of a sphere differs from  h^2 = rr - p^2  (p: the centre's distance from the ray's line) by at most
//       E(rr) = A S^2 + 2 eps rr,    A = 13 eps + 1.02 eta
//   and  RN(b - s) / RN(b + s)  of two spheres on one ray keep their order if the exact chords are nested with a margin  g = (16 eps + eta) S.
// Sphere X "encloses item I with the inflation" when
//       rr_X (1 - 2 eps) - A S^2  >=  ( |c_X - c_I| + sqrt(rr_I (1 + 2 eps) + A S^2) + g )^2 :
// then whenever the reference's test of I returns a finite distance d_I, its test of X returns a finite d_X, and d_X <= d_I if the origin
// is clearly outside X.
//   (a) B' encloses every item of the subtree with the inflation;
//   (b) so does the GIVEN sphere (a bound that leaves an item outside culls visibly in the reference, and only its own record does the same);
//   (c) the eye is clearly outside both spheres (the primary filter's threshold is finite for both: rt_skip.hpp primary_filter_threshold);
//   (d) B' is smaller than the given sphere by more than its own inflation, and its centre is no further from m0 than the given nodes' (the
//       shadow filter's constants stay valid for it).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include "rt_filter_bounds.hpp"

namespace rt_tight {

struct Params {
    double eye[3];      // Scene::eye
    double m0[3];       // FilterConsts::m0
    double rc;          // max |centre - m0| over the given nodes
    double S;           // >= |centre - origin| for every node and every ray origin of a render pass (the eye, shadow origins)
    double eta;         // >= | |d|^2 - 1 | for every ray direction (primary: 16 eps; shadow: FilterConsts::eta)
};

struct Result {
    std::vector<float> sphere;      // 4 per node: what the tight stream carries (ITEM nodes and rejected BOUND nodes: the given values, bit for bit)
    std::vector<uint8_t> tight;     // per node: 1 = a BOUND that carries B'
    uint32_t n_bounds = 0, n_tight = 0;
    double volume_ratio = 1.0;      // sum of r'^3 over sum of r^3 of the BOUND nodes (1: nothing gained)
};

constexpr double kEps = 0x1p-24;

struct Ball { double c[3], r; };

inline double dist3(const double *a, const double *b)
{
    return std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
}

// An enclosing ball of `balls` (not the smallest one: within a fraction of a percent after `steps` Badoiu-Clarkson steps; the best iterate is kept).
inline Ball enclosing_ball(const std::vector<Ball> &balls, int steps)
{
    Ball cur = balls[0], best = balls[0];
    best.r = INFINITY;
    int last_gain = 0;
    for (int k = 1; k <= steps; ++k) {
        double far = -1.0; size_t fi = 0;
        for (size_t j = 0; j < balls.size(); ++j) {
            const double d = dist3(cur.c, balls[j].c) + balls[j].r;
            if (d > far) { far = d; fi = j; }
        }
        if (far < best.r * (1.0 - 1e-7)) last_gain = k;
        if (far < best.r) { best = cur; best.r = far; }
        if (k - last_gain >= 48) break;                      // nothing gained for a while: converged as far as these steps go
        const double t = 1.0 / (k + 1.0);
        for (int a = 0; a < 3; ++a) cur.c[a] += (balls[fi].c[a] - cur.c[a]) * t;
    }
    return best;
}

inline float round_up(double v)
{
    float f = (float)v;
    if ((double)f < v) f = std::nextafterf(f, INFINITY);
    return f;
}

// sph: {cx, cy, cz, r} per node; skip: 0 for an ITEM, else the index of the first node behind the BOUND's subtree (DFS pre-order).
inline void build(const float *sph, const uint32_t *skip, uint32_t n, const Params &p, Result &out, int steps = 200)
{
    out.sphere.assign(sph, sph + (size_t)4 * n);
    out.tight.assign(n, 0);
    out.n_bounds = out.n_tight = 0;
    const double A = 13.0 * kEps + 1.02 * p.eta, AS2 = A * p.S * p.S, g = (16.0 * kEps + p.eta) * p.S;
    // Cost: every BOUND looks at every item of its subtree two or three times -- O(nodes x depth), a few tens of milliseconds for the 27,000 nodes
    // of the default scene, and quadratic on a hierarchy that degenerates into a chain.  `budget` caps it: a scene that runs out gets no tight
    // spheres at all (the caller then makes no tight streams), never a wrong one.
    uint64_t budget = (uint64_t)512 * n + 1000000u;
    bool out_of_budget = false;
    // the radius a sphere around `c` needs to enclose the items of [first, last) with the inflation, and without it
    auto needed = [&](const double *c, uint32_t first, uint32_t last, double &plain) {
        double q = 0.0; plain = 0.0;
        if (budget < last - first) { out_of_budget = true; plain = INFINITY; return (double)INFINITY; }
        budget -= last - first;
        for (uint32_t j = first; j < last; ++j) {
            if (skip[j] != 0u) continue;
            const double ci[3] = { sph[4 * j], sph[4 * j + 1], sph[4 * j + 2] }, ri = sph[4 * j + 3];
            const double D = dist3(c, ci);
            plain = std::max(plain, D + ri);
            q = std::max(q, D + std::sqrt(ri * ri * (1.0 + 2.0 * kEps) + AS2) + g);
        }
        return std::sqrt((q * q + AS2) / (1.0 - 2.0 * kEps)) * (1.0 + 1e-12);
    };
    // the eye clearly outside {c, r} as the device sees it: primary_filter_threshold's condition with a factor of two in hand
    // (vv here is exact for the f32 differences; the stream's is within 3 eps of it)
    auto eye_outside = [&](const float *c, float r) {
        const double v[3] = { (double)(float)(c[0] - (float)p.eye[0]), (double)(float)(c[1] - (float)p.eye[1]), (double)(float)(c[2] - (float)p.eye[2]) };
        const double vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], rr = (double)r * (double)r;
        return vv >= 4e-14 && vv - rr >= 128.0 * kEps * (vv + rr);
    };
    std::vector<Ball> ball(n);              // per node: a ball known to enclose the subtree's items (r < 0: none known)
    std::vector<Ball> kids;
    double vol_given = 0.0, vol_tight = 0.0;
    for (uint32_t i = n; i-- > 0;) {
        const double ci[3] = { sph[4 * i], sph[4 * i + 1], sph[4 * i + 2] };
        if (skip[i] == 0u) { ball[i] = Ball{ { ci[0], ci[1], ci[2] }, (double)sph[4 * i + 3] }; continue; }
        ++out.n_bounds;
        const uint32_t last = skip[i];
        const double r_given = sph[4 * i + 3];
        vol_given += r_given * r_given * r_given; vol_tight += r_given * r_given * r_given;
        double plain_g;
        const bool b_ok = r_given >= needed(ci, i + 1, last, plain_g);                       // (b)
        ball[i] = Ball{ { ci[0], ci[1], ci[2] }, r_given >= plain_g ? r_given : -1.0 };
        if (out_of_budget) break;
        // a node that fails (b) or (c) with the sphere it was given keeps it whatever B' would be: no enclosing-ball steps for it (a hierarchy
        // built tightly around its items fails (b) at every node, and costs one pass over each subtree)
        if (!b_ok || !eye_outside(&sph[4 * i], sph[4 * i + 3])) continue;
        kids.clear();
        bool all_known = true;
        for (uint32_t c = i + 1; c < last; c = skip[c] ? skip[c] : c + 1u) { kids.push_back(ball[c]); all_known = all_known && ball[c].r >= 0.0; }
        if (!all_known) {                    // a child group without a known enclosing ball: over the subtree's items themselves
            kids.clear();
            for (uint32_t j = i + 1; j < last; ++j) if (skip[j] == 0u) kids.push_back(ball[j]);
        }
        if (kids.empty()) continue;
        const uint64_t ball_work = (uint64_t)kids.size() * (uint64_t)steps / 4u;             // (the enclosing-ball steps count as well)
        if (budget < ball_work) { out_of_budget = true; break; }
        budget -= ball_work;
        const Ball cand = enclosing_ball(kids, steps);
        const float cf[3] = { (float)cand.c[0], (float)cand.c[1], (float)cand.c[2] };
        const double cd[3] = { cf[0], cf[1], cf[2] };
        double plain_t;
        const double need_t = needed(cd, i + 1, last, plain_t);                              // (a), by construction of the radius
        const float rf = round_up(need_t);
        if (plain_t < (ball[i].r >= 0.0 ? ball[i].r : INFINITY)) ball[i] = Ball{ { cd[0], cd[1], cd[2] }, plain_t * (1.0 + 1e-12) };
        if (out_of_budget) break;
        if (!std::isfinite(rf)) continue;
        if (!eye_outside(cf, rf)) continue;                                                  // (c)
        if (!(r_given - (double)rf > (double)rf - plain_t)) continue;                        // (d)
        if (!(dist3(cd, p.m0) <= p.rc)) continue;
        out.sphere[4 * i] = cf[0]; out.sphere[4 * i + 1] = cf[1]; out.sphere[4 * i + 2] = cf[2]; out.sphere[4 * i + 3] = rf;
        out.tight[i] = 1; ++out.n_tight;
        vol_tight += (double)rf * rf * rf - r_given * r_given * r_given;
    }
    if (out_of_budget) {
        out.sphere.assign(sph, sph + (size_t)4 * n);
        out.tight.assign(n, 0);
        out.n_tight = 0; vol_tight = vol_given;
    }
    out.volume_ratio = vol_given > 0.0 ? vol_tight / vol_given : 1.0;
}

// ---- Per-walk records (NOTES.md "Per-walk bounds") --------------------------------------------------------------------------------------
// The tight ball serves both walks; neither needs a ball for its quiet decision.  Primary rays share the eye: their filter is a cone from the
// eye about the node's v.  Shadow rays share the direction: their filter is a disc in the plane across the light.  For every BOUND that
// carries a tight ball, build_walk computes
//   an EYE SPHERE {c', r'}: c' on the axis of the narrowest cap (seen from the eye) that holds every item's cap -- an item's cap is what its
//       own primary_threshold admits --, r' what rules (a) and (c) above need, |c' - m0| <= rc; the exact test of the primary walk runs on it;
//   T': finite distance_from_ray for any item of the subtree implies  fma(v'z, dz, fma(v'y, dy, v'x dx)) >= T'  (v' = fl(c' - eye));
//   Rq: that fma chain b' minus Rq is no larger than the reference's distance to the eye sphere, hence to any item of the subtree
//       (rt_filter_bounds.hpp lean_radius): the lean BOUND step of the primary loop enters iff b' >= T' and b' - Rq < hit.distance;
//   a LIGHT DISC {w1', w2', R2o'}: P2' > R2o' as the loops form it implies P2_I > R2o_I for every item, which implies that the reference says MISS;
//   its FRONT cl': fl(cl' - ol) <= -a0 implies that every item fulfils its own behind-the-origin test (the loops' second chance reads cl);
//   R2i': the disc of that radius about (w1', w2') lies inside the tight ball's inner disc (-1: no room).
// A record is kept only where it is narrower than what the tight ball gives the same walk.  The exact shadow record stays the tight ball's.
struct WalkParams {
    Params base;
    float eye[3];                   // Scene::eye as the stream kernels see it
    float m0[3], e1[3], e2[3], l[3];    // FilterConsts
    double fS, feta;                // FilterConsts::S, ::eta
};

struct WalkResult {
    std::vector<float> eye_sphere;              // 4 per node: the raw sphere of the primary per-walk stream (no record: the tight stream's)
    std::vector<rt_bounds::WalkOverride> ovr;   // per node (flags 0: none)
    uint32_t n_primary = 0, n_shadow = 0;       // BOUNDs that carry an eye sphere / a light disc
    double cone_ratio = 1.0, disc_ratio = 1.0;  // mean half-angle / disc radius of the records kept, relative to the tight ball's
};

inline float round_down(double v)
{
    float f = (float)v;
    if ((double)f > v) f = std::nextafterf(f, -INFINITY);
    return f;
}

// slack: false makes the records of the plain geometry -- the items' silhouette caps and own discs, no rounding term in T', R2o' and cl'
// (tests only: on such records the rim fixtures must show violations).
// Cost: where the centres go is SEARCHED on a frontier of at most kWalkFrontier spheres of the tight stream (the node's children, the largest
// groups among them opened until there are that many); T', r', R2o' and cl' are then taken from one pass over every item of the subtree.
constexpr size_t kWalkFrontier = 24;
inline void build_walk(const float *sph, const uint32_t *skip, uint32_t n, const Result &tr, const WalkParams &wp, WalkResult &out, int steps = 32, bool slack = true)
{
    const Params &p = wp.base;
    out.eye_sphere = tr.sphere;
    out.ovr.assign(n, rt_bounds::WalkOverride{});
    out.n_primary = out.n_shadow = 0;
    out.cone_ratio = out.disc_ratio = 1.0;
    if (tr.n_tight == 0) return;
    const double eps = kEps, sl = slack ? 1.0 : 0.0;
    const double A = 13.0 * kEps + 1.02 * p.eta, AS2 = A * p.S * p.S, g = (16.0 * kEps + p.eta) * p.S;
    uint64_t budget = (uint64_t)512 * n + 1000000u;
    const double eye_d[3] = { wp.eye[0], wp.eye[1], wp.eye[2] };
    auto eye_outside = [&](const float *c, float r) {
        const double v[3] = { (double)(float)(c[0] - wp.eye[0]), (double)(float)(c[1] - wp.eye[1]), (double)(float)(c[2] - wp.eye[2]) };
        const double vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], rr = (double)r * (double)r;
        return vv >= 4e-14 && vv - rr >= 128.0 * kEps * (vv + rr);
    };
    // v = fl(c - eye), vv, rr and T of a sphere as k_build_streams / k_build_fstreams form them
    struct Seen { double v[3], len; float T; };
    auto seen_from_eye = [&](const float *c, float r) {
        const float vx = c[0] - wp.eye[0], vy = c[1] - wp.eye[1], vz = c[2] - wp.eye[2];
        const float vv = (vx * vx + vy * vy) + vz * vz, rr = r * r;
        Seen s{ { vx, vy, vz }, 0.0, rt_bounds::primary_threshold(vv, rr) };
        s.len = std::sqrt(s.v[0] * s.v[0] + s.v[1] * s.v[1] + s.v[2] * s.v[2]);
        return s;
    };
    // the centre in the plane across the light and along it, as k_build_fstreams forms it
    auto across_light = [&](const float *c, float &w1, float &w2, float &cl) {
        const double cx = (double)c[0] - (double)wp.m0[0], cy = (double)c[1] - (double)wp.m0[1], cz = (double)c[2] - (double)wp.m0[2];
        w1 = (float)((cx * (double)wp.e1[0] + cy * (double)wp.e1[1]) + cz * (double)wp.e1[2]);
        w2 = (float)((cx * (double)wp.e2[0] + cy * (double)wp.e2[1]) + cz * (double)wp.e2[2]);
        cl = (float)((cx * (double)wp.l[0] + cy * (double)wp.l[1]) + cz * (double)wp.l[2]);
    };
    // ---- every item once: its cap from the eye and its outer disc across the light, from the values its own records will carry ----
    struct ItemSeen {
        double c[3], r, infl;       // the sphere; sqrt(rr (1 + 2 eps) + A S^2) + g
        double v[3], len, ca, sa;   // fl(c - eye); cos / sin of the cap's half angle
        double w[2], rho, front;    // in-plane centre, sqrt(R2o), the plane behind which an origin passes the item's own second chance
        bool cap;                   // the item has a cap (its T is finite and positive)
    };
    std::vector<ItemSeen> seen(n);
    for (uint32_t j = 0; j < n; ++j) {
        if (skip[j] != 0u) continue;
        ItemSeen &it = seen[j];
        const Seen s = seen_from_eye(&sph[4 * j], sph[4 * j + 3]);
        for (int a = 0; a < 3; ++a) { it.v[a] = s.v[a]; it.c[a] = sph[4 * j + a]; }
        it.r = sph[4 * j + 3]; it.len = s.len;
        it.infl = std::sqrt(it.r * it.r * (1.0 + 2.0 * kEps) + AS2) + g;
        // the item's cap: finite implies b'_I >= T_I; b'_I is within 4 eps |v_I| of v_I . d; |d| <= 1 + 8.1 eps
        const double ci = std::isfinite(s.T) && s.len > 0.0 ? ((double)s.T - sl * 4.0 * eps * s.len) / (s.len * (1.0 + sl * 9.0 * eps)) : -1.0;
        it.cap = ci > 0.0;
        it.ca = std::min(ci, 1.0); it.sa = std::sqrt(std::max(0.0, 1.0 - it.ca * it.ca));
        float w1, w2, cl, r2o, r2i;
        across_light(&sph[4 * j], w1, w2, cl);
        const float rr = sph[4 * j + 3] * sph[4 * j + 3];
        rt_bounds::shadow_bounds(wp.fS, wp.feta, rr, r2o, r2i);
        it.w[0] = w1; it.w[1] = w2; it.rho = std::sqrt((double)r2o);
        // a <= -a0 and (P2 + a^2) kc >= R2o with kc = 1 / (1 + 2^-8): behind this plane an origin fulfils the item's own second chance
        it.front = (double)cl + it.rho * std::sqrt(1.0 + 0x1p-8) * (1.0 + sl * 8.0 * eps);
        if (!slack) {                // the plain geometry: the silhouette's cap, the sphere's own disc and front
            const double vv = it.len * it.len, rr = it.r * it.r;
            it.cap = vv > rr;
            it.sa = it.cap ? it.r / it.len : 1.0; it.ca = std::sqrt(std::max(0.0, 1.0 - it.sa * it.sa));
            it.rho = it.r; it.front = (double)cl + it.r;
        }
    }
    struct Proxy { double c[3], r, u[3], ca, sa, w[2], rho; };
    std::vector<uint32_t> frontier;
    std::vector<Proxy> prox;
    std::vector<Ball> discs;
    double cone_sum = 0.0, disc_sum = 0.0;
    bool out_of_budget = false;
    for (uint32_t i = 0; i < n; ++i) {
        if (skip[i] == 0u || !tr.tight[i]) continue;
        const uint32_t last = skip[i];
        const uint64_t work = (uint64_t)(last - i - 1u) + (uint64_t)kWalkFrontier * (uint64_t)steps;
        if (budget < work) { out_of_budget = true; break; }
        budget -= work;
        const float *ball = &tr.sphere[4 * i];
        // ---- the frontier the centres are searched on ----
        frontier.clear();
        for (uint32_t c = i + 1; c < last; c = skip[c] ? skip[c] : c + 1u) frontier.push_back(c);
        while (frontier.size() < kWalkFrontier) {
            size_t big = frontier.size();
            for (size_t k = 0; k < frontier.size(); ++k)
                if (skip[frontier[k]] != 0u && (big == frontier.size() || tr.sphere[4 * frontier[k] + 3] > tr.sphere[4 * frontier[big] + 3])) big = k;
            if (big == frontier.size()) break;
            const uint32_t b = frontier[big];
            frontier[big] = frontier.back(); frontier.pop_back();
            for (uint32_t c = b + 1; c < skip[b]; c = skip[c] ? skip[c] : c + 1u) frontier.push_back(c);
        }
        if (frontier.empty()) continue;
        prox.clear();
        for (uint32_t f : frontier) {
            Proxy q{};
            double len = 0.0;
            for (int a = 0; a < 3; ++a) { q.c[a] = tr.sphere[4 * f + a]; q.u[a] = q.c[a] - eye_d[a]; len += q.u[a] * q.u[a]; }
            len = std::sqrt(len); q.r = tr.sphere[4 * f + 3];
            for (int a = 0; a < 3; ++a) q.u[a] = len > 0.0 ? q.u[a] / len : 0.0;
            q.sa = len > 0.0 ? std::min(1.0, q.r / len) : 1.0; q.ca = std::sqrt(1.0 - q.sa * q.sa);
            float w1, w2, cl;
            across_light(&tr.sphere[4 * f], w1, w2, cl);
            q.w[0] = w1; q.w[1] = w2; q.rho = q.r;
            prox.push_back(q);
        }
        const Seen sb = seen_from_eye(ball, ball[3]);
        bool caps = true;
        for (uint32_t j = i + 1; j < last; ++j) if (skip[j] == 0u && !seen[j].cap) { caps = false; break; }
        rt_bounds::WalkOverride o{};
        // ---------------- the eye sphere and T' ----------------
        while (caps && std::isfinite(sb.T) && sb.T > 0.0f) {
            // the axis of the narrowest cap that holds the frontier's caps: enclosing-ball steps on the direction sphere (the cosine of
            // "angle to the far rim" is the smallest cos(phi + alpha))
            double ax[3] = { sb.v[0] / sb.len, sb.v[1] / sb.len, sb.v[2] / sb.len }, bax[3] = { ax[0], ax[1], ax[2] }, best = -2.0;
            for (int k = 1; k <= steps; ++k) {
                double far = 2.0; size_t fi = 0;
                for (size_t j = 0; j < prox.size(); ++j) {
                    const double cp = std::min(1.0, ax[0] * prox[j].u[0] + ax[1] * prox[j].u[1] + ax[2] * prox[j].u[2]);
                    const double d = cp * prox[j].ca - std::sqrt(std::max(0.0, 1.0 - cp * cp)) * prox[j].sa;
                    if (d < far) { far = d; fi = j; }
                }
                if (far > best) { best = far; bax[0] = ax[0]; bax[1] = ax[1]; bax[2] = ax[2]; }
                const double t = 1.0 / (k + 1.0);
                double len = 0.0;
                for (int a = 0; a < 3; ++a) { ax[a] += (prox[fi].u[a] - ax[a]) * t; len += ax[a] * ax[a]; }
                len = std::sqrt(len);
                if (!(len > 0.0)) break;
                for (int a = 0; a < 3; ++a) ax[a] /= len;
            }
            // the smallest ball centred on that axis that holds the frontier: a convex function of the position along it
            double lo = INFINITY, hi = -INFINITY;
            for (const Proxy &q : prox) {
                const double t = (q.c[0] - eye_d[0]) * bax[0] + (q.c[1] - eye_d[1]) * bax[1] + (q.c[2] - eye_d[2]) * bax[2];
                lo = std::min(lo, t - q.r); hi = std::max(hi, t + q.r);
            }
            auto radius_at = [&](double t) {
                const double c[3] = { eye_d[0] + t * bax[0], eye_d[1] + t * bax[1], eye_d[2] + t * bax[2] };
                double r = 0.0;
                for (const Proxy &q : prox) r = std::max(r, dist3(c, q.c) + q.r);
                return r;
            };
            for (int k = 0; k < 20; ++k) {
                const double m1 = lo + (hi - lo) / 3.0, m2 = hi - (hi - lo) / 3.0;
                if (radius_at(m1) < radius_at(m2)) hi = m2; else lo = m1;
            }
            const double tc = 0.5 * (lo + hi);
            const float cf[3] = { (float)(eye_d[0] + tc * bax[0]), (float)(eye_d[1] + tc * bax[1]), (float)(eye_d[2] + tc * bax[2]) };
            const double cd[3] = { cf[0], cf[1], cf[2] };
            const Seen sx = seen_from_eye(cf, 0.0f);       // (v' and its length; T comes with the radius)
            if (!(sx.len > 0.0)) break;
            // one pass over the items: rule (a)'s radius, and every item's cap about the node's OWN v (cos(phi + alpha), phi from the cross product)
            double q = 0.0, cmin = 1.0;
            for (uint32_t j = i + 1; j < last; ++j) {
                if (skip[j] != 0u) continue;
                const ItemSeen &it = seen[j];
                q = std::max(q, dist3(cd, it.c) + it.infl);
                const double cx = sx.v[1] * it.v[2] - sx.v[2] * it.v[1], cy = sx.v[2] * it.v[0] - sx.v[0] * it.v[2], cz = sx.v[0] * it.v[1] - sx.v[1] * it.v[0];
                const double nn = sx.len * it.len;
                const double cp = (sx.v[0] * it.v[0] + sx.v[1] * it.v[1] + sx.v[2] * it.v[2]) / nn, sp = std::sqrt(cx * cx + cy * cy + cz * cz) / nn;
                cmin = std::min(cmin, cp * it.ca - sp * it.sa);
                if (cp <= 0.0) cmin = -1.0;                  // (more than a right angle off the axis: no record)
            }
            const float rf = round_up(std::sqrt((q * q + AS2) / (1.0 - 2.0 * kEps)) * (1.0 + 1e-12));
            if (!std::isfinite(rf) || !eye_outside(cf, rf) || !(dist3(cd, p.m0) <= p.rc)) break;      // rule (c); S covers the centre
            const Seen sr = seen_from_eye(cf, rf);
            if (!std::isfinite(sr.T)) break;
            if (!(cmin > 0.1)) break;
            const double theta = std::acos(std::min(1.0, cmin)) + sl * 1e-9;
            // v' . d = |v'| |d| cos(angle) >= |v'| (1 - 8.1 eps) cos(theta); b' is within 4 eps |v'| of it; rounded down twice
            const double tpd = sx.len * ((1.0 - sl * 9.0 * eps) * std::cos(theta) - sl * 4.0 * eps) - sl * 1e-44;
            float tp = round_down(tpd);
            if (slack) tp = std::nextafterf(tp, -INFINITY);
            const double cos_new = std::max((double)tp, (double)sr.T) / sx.len, cos_ball = (double)sb.T / sb.len;
            if (!(cos_new > cos_ball) || !(cos_new < 1.0)) break;      // keep it only where the cone is narrower than the tight ball's
            out.eye_sphere[4 * i] = cf[0]; out.eye_sphere[4 * i + 1] = cf[1]; out.eye_sphere[4 * i + 2] = cf[2]; out.eye_sphere[4 * i + 3] = rf;
            o.tp = tp; o.flags |= rt_bounds::kWalkPrimary;
            {   // Rq from vv and rr as k_build_streams forms them for this sphere (the lean BOUND step, NOTES.md "Lean bound steps")
                const float vx = cf[0] - wp.eye[0], vy = cf[1] - wp.eye[1], vz = cf[2] - wp.eye[2];
                o.rq = rt_bounds::lean_radius((vx * vx + vy * vy) + vz * vz, rf * rf, AS2);
            }
            ++out.n_primary;
            cone_sum += std::acos(cos_new) / std::acos(std::min(1.0, std::max(cos_ball, 0.0)));
            break;
        }
        // ---------------- the light disc ----------------
        do {
            float bw1, bw2, bcl, br2o, br2i;
            across_light(ball, bw1, bw2, bcl);
            rt_bounds::shadow_bounds(wp.fS, wp.feta, ball[3] * ball[3], br2o, br2i);
            discs.clear();
            for (const Proxy &q : prox) discs.push_back(Ball{ { q.w[0], q.w[1], 0.0 }, q.rho });
            const Ball e = enclosing_ball(discs, steps);
            const float w1 = (float)e.c[0], w2 = (float)e.c[1];
            double R = 0.0, front = -INFINITY;
            for (uint32_t j = i + 1; j < last; ++j) {
                if (skip[j] != 0u) continue;
                const ItemSeen &it = seen[j];
                const double dx = (double)w1 - it.w[0], dy = (double)w2 - it.w[1];
                R = std::max(R, std::sqrt(dx * dx + dy * dy) + it.rho);
                front = std::max(front, it.front);
            }
            // P2' <= rho'^2 (1 + eps)^2 (1 + 2.01 eps) and P2_I >= rho_I^2 (1 - eps)^2 (1 - 2.01 eps) for the exact in-plane distances rho of the
            // rounded coordinates; rho_I >= rho' - |w' - w_I|; 4 eps S: the item centres as another compiler may round them
            R += sl * 4.0 * eps * wp.fS;
            float r2o = round_up(R * R * (1.0 + sl * 16.0 * eps) + sl * 1e-36);
            if (slack) r2o = std::nextafterf(r2o, INFINITY);
            if (!std::isfinite(r2o) || !(r2o < br2o)) break;                               // keep it only where the disc is smaller than the tight ball's
            const float cl = round_up(front + sl * 16.0 * eps * wp.fS);
            if (!std::isfinite(cl) || !std::isfinite(w1) || !std::isfinite(w2)) break;
            float r2i = -1.0f;
            if (br2i > 0.0f) {
                const double dx = (double)w1 - (double)bw1, dy = (double)w2 - (double)bw2;
                const double ri = std::sqrt((double)br2i) - std::sqrt(dx * dx + dy * dy) - 4.0 * eps * wp.fS;
                if (ri > 0.0) {
                    const float f = std::nextafterf(round_down(ri * ri * (1.0 - 16.0 * eps)), -INFINITY);
                    if (f > 0.0f) r2i = f;
                }
            }
            o.w1 = w1; o.w2 = w2; o.cl = cl; o.r2o = r2o; o.r2i = r2i; o.flags |= rt_bounds::kWalkShadow;
            ++out.n_shadow;
            disc_sum += std::sqrt((double)r2o / (double)br2o);
        } while (false);
        out.ovr[i] = o;
    }
    if (out_of_budget) {
        out.eye_sphere = tr.sphere;
        out.ovr.assign(n, rt_bounds::WalkOverride{});
        out.n_primary = out.n_shadow = 0;
        return;
    }
    if (out.n_primary) out.cone_ratio = cone_sum / out.n_primary;
    if (out.n_shadow) out.disc_ratio = disc_sum / out.n_shadow;
}

}  // namespace rt_tight
