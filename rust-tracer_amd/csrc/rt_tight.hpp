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

}  // namespace rt_tight
