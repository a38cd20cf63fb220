// tools/step_census.cpp -- design-time estimator, not part of the product and not a parity oracle.
//
// Census of the step types of the fused, filtered skip-pointer walk for every 8x8-pixel wave of a frame of the default scene (primary:
// quiet / BOUND with a candidate that nobody enters / entered, own sphere quiet / entered, own sphere a candidate / ITEM candidate;
// shadow: quiet / hit) with the vector instructions each costs in rt_skip_rot.hpp, and of the primary BOUND steps that the root-free
// decision of round 4 settles (rt_skip.hpp bound_shortcut_verdict: b <= 0, b < hit.distance, disc (1 + 2^-20) <= RN(b - hit.distance)^2) --
// checking on the way that the verdict never contradicts the reference's `d >= hit.distance`.
//
// --tight: the un-fused walk over the tight bounds of rt_tight.hpp (a BOUND's own sphere is the ITEM step behind it), the prediction the
// GPU numbers of the tight streams are read against; the hash of every pixel's hit item and shadow verdict must equal the plain run's.
//
// --walk: the same walk over the per-walk records of rt_tight.hpp build_walk -- primary: a BOUND carries its eye sphere and max(T of it, T'),
// a lane sleeps where the fused chain b' stays below that or the reference's test of the eye sphere culls; shadow: a BOUND carries its light
// disc, a lane sleeps where P2 > R2o' or the front says "behind the origin", enters where the inner disc says so, and runs the reference's
// test of the TIGHT ball in between.  A step is quiet when no live lane passes the node's filter.  The hash must equal the other runs'.
// Both print the steps of the heaviest waves and the longest single pixel.
//
// --lean: the --walk records with the lean BOUND step (NOTES.md "Lean bound steps"): a BOUND with an eye sphere is decided by the filter's b'
// and the library's own Rq (rt_filter_bounds.hpp lean_radius) -- a lane enters iff b' >= T' and b' - Rq < hit.distance --, every other node as
// under --walk.  Prints the split of the candidate BOUND steps and complains on stderr if a lane sleeps at an ITEM the exact test makes a winner.
//
//   g++ -O2 -ffp-contract=off -o /tmp/step_census tools/step_census.cpp && /tmp/step_census [w h [level]] [--tight | --walk | --lean]
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../rust-tracer_amd/csrc/rt_tight.hpp"
struct V3 { float x, y, z; };
static inline V3 add(V3 a, V3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
static inline V3 sub(V3 a, V3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
static inline V3 mulf(V3 a, float m) { return { a.x * m, a.y * m, a.z * m }; }
static inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline V3 normalized(V3 a) { float l = sqrtf(dot(a, a)); return mulf(a, 1.0f / l); }
struct Node { V3 c; float r; uint32_t skip; int item; };
// --walk: what the filter streams carry for a node (k_build_fstreams with the records of build_walk)
struct Filt { V3 pc; float pr, f5, w1, w2, cl, r2o, r2i, rq; };      // rq > 0: a lean BOUND (--lean)
static std::vector<Filt> filt;
static std::vector<Node> nodes;
static void pyramid(unsigned level, V3 p, float r)
{
    if (level == 1) { nodes.push_back({ p, r, (uint32_t)nodes.size() + 1, 1 }); return; }
    const int me = (int)nodes.size();
    nodes.push_back({ p, 3.0f * r, 0, 0 });
    nodes.push_back({ p, r, (uint32_t)nodes.size() + 1, 1 });
    const float rn = 3.0f * r / sqrtf(12.0f);
    const int sgn[2] = { -1, 1 };
    for (int iz = 0; iz < 2; ++iz) for (int ix = 0; ix < 2; ++ix) pyramid(level - 1, add(p, { sgn[ix] * rn, rn, sgn[iz] * rn }), r * 0.5f);
    nodes[me].skip = (uint32_t)nodes.size();
}
static inline float dist(V3 c, float r, V3 o, V3 d, float *disc_out)
{
    const V3 v = sub(c, o); const float b = dot(v, d); const float disc = b * b - dot(v, v) + r * r; *disc_out = disc;
    if (disc < 0.0f) return INFINITY; const float s = sqrtf(disc); const float t2 = b + s; if (t2 < 0.0f) return INFINITY; const float t1 = b - s; return t1 > 0.0f ? t1 : t2;
}
int main(int argc, char **argv)
{
    bool tight = false, walk = false, lean = false;
    std::vector<char *> pos;
    for (int a = 1; a < argc; ++a) { if (!strcmp(argv[a], "--tight")) tight = true; else if (!strcmp(argv[a], "--walk")) tight = walk = true; else if (!strcmp(argv[a], "--lean")) tight = walk = lean = true; else pos.push_back(argv[a]); }
    float fq_m0[3] = { 0, 0, 0 }, fq_e1[3] = { 0, 0, 0 }, fq_e2[3] = { 0, 0, 0 }, fq_l[3] = { 0, 0, 0 }, fq_a0 = 0, fq_k1 = 0, fq_kc = 0;
    const unsigned W = pos.size() > 0 ? atoi(pos[0]) : 1920, H = pos.size() > 1 ? atoi(pos[1]) : 1080, level = pos.size() > 2 ? atoi(pos[2]) : 8;
    pyramid(level, { 0, -1, 0 }, 1.0f);
    const size_t n = nodes.size();
    const V3 eye = { 0, 0, -4 }, light = normalized({ -1, -3, 2 }), sdir = mulf(light, -1.0f);
    if (tight) {
        // the constants rt_scene_create hands rt_tight::build (rt_capi_scene.hpp filter_constants, tight_params)
        std::vector<float> sph(4 * n); std::vector<uint32_t> skip(n);
        double m0[3] = { 0, 0, 0 }; size_t n_items = 0;
        for (size_t i = 0; i < n; ++i) {
            sph[4 * i] = nodes[i].c.x; sph[4 * i + 1] = nodes[i].c.y; sph[4 * i + 2] = nodes[i].c.z; sph[4 * i + 3] = nodes[i].r; skip[i] = nodes[i].item ? 0u : nodes[i].skip;
            if (nodes[i].item) { m0[0] += nodes[i].c.x; m0[1] += nodes[i].c.y; m0[2] += nodes[i].c.z; ++n_items; }
        }
        rt_tight::Params p{};
        for (int k = 0; k < 3; ++k) p.m0[k] = (double)(float)(m0[k] / (double)n_items);
        p.eye[0] = eye.x; p.eye[1] = eye.y; p.eye[2] = eye.z;
        double rc = 0, rit = 0;
        for (size_t i = 0; i < n; ++i) {
            const double c[3] = { nodes[i].c.x, nodes[i].c.y, nodes[i].c.z }, d = rt_tight::dist3(c, p.m0);
            rc = std::max(rc, d); if (nodes[i].item) rit = std::max(rit, d + nodes[i].r);
        }
        const double eye_d = rt_tight::dist3(p.eye, p.m0);
        const double ro = 1.01 * rit + 1e-3 * (eye_d + rit) + 1e-5 * (fabs(p.eye[0]) + fabs(p.eye[1]) + fabs(p.eye[2]) + fabs(p.m0[0]) + fabs(p.m0[1]) + fabs(p.m0[2]));
        const double l2 = (double)sdir.x * sdir.x + (double)sdir.y * sdir.y + (double)sdir.z * sdir.z;
        p.rc = rc; p.S = std::max(rc + ro * (1.0 + 4.0 * rt_tight::kEps), rc + eye_d) * (1.0 + 1e-9); p.eta = std::max(16.0 * rt_tight::kEps, fabs(l2 - 1.0));
        rt_tight::Result tr;
        rt_tight::build(sph.data(), skip.data(), (uint32_t)n, p, tr);
        for (size_t i = 0; i < n; ++i) if (tr.tight[i]) { nodes[i].c = { tr.sphere[4 * i], tr.sphere[4 * i + 1], tr.sphere[4 * i + 2] }; nodes[i].r = tr.sphere[4 * i + 3]; }
        printf("tight: %u of %u bounds carry a tight sphere, volume ratio %.4f (S %.4f)\n", tr.n_tight, tr.n_bounds, tr.volume_ratio, p.S);
        if (walk) {
            // the shadow filter's frame and constants (rt_capi_scene.hpp filter_constants), then the library's own build_walk
            rt_tight::WalkParams wp{};
            wp.base = p;
            const double l[3] = { sdir.x, sdir.y, sdir.z }, ln = sqrt(l2), lh[3] = { l[0] / ln, l[1] / ln, l[2] / ln };
            int ax = 0;
            for (int k = 1; k < 3; ++k) if (fabs(lh[k]) < fabs(lh[ax])) ax = k;
            double a[3] = { 0, 0, 0 }; a[ax] = 1.0;
            double e1[3] = { lh[1] * a[2] - lh[2] * a[1], lh[2] * a[0] - lh[0] * a[2], lh[0] * a[1] - lh[1] * a[0] };
            const double n1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
            for (int k = 0; k < 3; ++k) e1[k] /= n1;
            const double e2[3] = { lh[1] * e1[2] - lh[2] * e1[1], lh[2] * e1[0] - lh[0] * e1[2], lh[0] * e1[1] - lh[1] * e1[0] };
            const float eyef[3] = { eye.x, eye.y, eye.z };
            for (int k = 0; k < 3; ++k) { wp.eye[k] = eyef[k]; wp.m0[k] = fq_m0[k] = (float)p.m0[k]; wp.e1[k] = fq_e1[k] = (float)e1[k]; wp.e2[k] = fq_e2[k] = (float)e2[k]; wp.l[k] = fq_l[k] = (float)l[k]; }
            wp.feta = fabs(l2 - 1.0); wp.fS = (rc + ro * (1.0 + 4.0 * rt_tight::kEps)) * (1.0 + 1e-9);
            auto up = [](double v) { float f = (float)v; if ((double)f < v) f = nextafterf(f, INFINITY); return nextafterf(f, INFINITY); };
            fq_a0 = up(11.0 * rt_tight::kEps * wp.fS + 1e-37);
            fq_k1 = up((wp.feta + 10.2 * rt_tight::kEps) * (1.0 + wp.feta) * (1.0 + 12.0 * rt_tight::kEps));
            { float kc = (float)(1.0 / (1.0 + 4.0 * 0x1p-10)); if ((double)kc > 1.0 / (1.0 + 4.0 * 0x1p-10)) kc = nextafterf(kc, 0.0f); fq_kc = nextafterf(kc, 0.0f); }
            rt_tight::WalkResult wr;
            rt_tight::build_walk(tr.sphere.data(), skip.data(), (uint32_t)n, tr, wp, wr);
            printf("walk: %u eye spheres, %u light discs of %u tight bounds; cone half-angle %.3f, disc radius %.3f of the tight ball's\n", wr.n_primary, wr.n_shadow, tr.n_tight, wr.cone_ratio, wr.disc_ratio);
            filt.resize(n);
            for (size_t i = 0; i < n; ++i) {
                Filt &f = filt[i];
                const rt_bounds::WalkOverride &o = wr.ovr[i];
                f.pc = { wr.eye_sphere[4 * i], wr.eye_sphere[4 * i + 1], wr.eye_sphere[4 * i + 2] }; f.pr = wr.eye_sphere[4 * i + 3];
                const V3 v = sub(f.pc, eye);
                f.f5 = rt_bounds::primary_threshold((v.x * v.x + v.y * v.y) + v.z * v.z, f.pr * f.pr);
                if ((o.flags & rt_bounds::kWalkPrimary) && f.f5 > -INFINITY && o.tp > f.f5) f.f5 = o.tp;
                f.rq = (lean && !nodes[i].item && (o.flags & rt_bounds::kWalkPrimary) && f.f5 > -INFINITY && o.rq > 0.0f) ? o.rq : 0.0f;      // (k_build_fstreams, `lean`)
                const double cx = (double)nodes[i].c.x - (double)fq_m0[0], cy = (double)nodes[i].c.y - (double)fq_m0[1], cz = (double)nodes[i].c.z - (double)fq_m0[2];
                f.w1 = (float)((cx * (double)fq_e1[0] + cy * (double)fq_e1[1]) + cz * (double)fq_e1[2]);
                f.w2 = (float)((cx * (double)fq_e2[0] + cy * (double)fq_e2[1]) + cz * (double)fq_e2[2]);
                f.cl = (float)((cx * (double)fq_l[0] + cy * (double)fq_l[1]) + cz * (double)fq_l[2]);
                rt_bounds::shadow_bounds(wp.fS, wp.feta, nodes[i].r * nodes[i].r, f.r2o, f.r2i);
                if (o.flags & rt_bounds::kWalkShadow) { f.w1 = o.w1; f.w2 = o.w2; f.cl = o.cl; f.r2o = o.r2o; f.r2i = o.r2i; }
            }
        }
    }
    std::vector<uint32_t> wave_steps;
    unsigned longest_px = 0;
    uint64_t hash = 1469598103934665603ull;
    uint64_t pQ = 0, pB0 = 0, pB1 = 0, pB2 = 0, pI = 0, pLeafQ = 0, sQ = 0, sH = 0, sEnt = 0, waves = 0, swaves = 0;
    uint64_t pL0 = 0, pL1 = 0, lean_wrong = 0;   // --lean: candidate steps at lean BOUNDs nobody enters / somebody enters; sleeping lanes the exact test makes winners
    uint64_t dec1 = 0, dec2 = 0, dec1_b0 = 0;    // B0 steps in which every candidate lane has b >= best (root-free "no" possible) 
    for (unsigned y0 = 0; y0 < H; y0 += 8) for (unsigned x0 = 0; x0 < W; x0 += 8) {
        V3 dir[64]; bool in[64]; float best[64]; int bi[64]; uint32_t res[64]; unsigned awake[64]; uint32_t wsteps = 0;
        for (unsigned l = 0; l < 64; ++l) awake[l] = 0;
        for (unsigned l = 0; l < 64; ++l) { unsigned x = x0 + l % 8, y = y0 + l / 8; in[l] = x < W && y < H; dir[l] = normalized({ (float)x - W / 2.0f, ((float)H - (float)y) - H / 2.0f, (float)W }); best[l] = INFINITY; bi[l] = -1; res[l] = in[l] ? 0u : 0xFFFFFFFFu; }
        ++waves;
        for (size_t i = 0; i < n;) {
            const Node &nd = nodes[i];
            bool cand = false, enter = false, undecided = false, undecided2 = false;
            ++wsteps;
            for (unsigned l = 0; l < 64; ++l) {
                if (lean && nd.item && in[l] && i < res[l]) {      // asleep: the exact test must not make this item a winner
                    const Filt &f = filt[i]; const V3 v = sub(f.pc, eye); float xdisc;
                    if (f.f5 <= fmaf(v.z, dir[l].z, fmaf(v.y, dir[l].y, v.x * dir[l].x)) && !(dist(f.pc, f.pr, eye, dir[l], &xdisc) >= best[l])) {
                        if (!lean_wrong++) fprintf(stderr, "LEAN SLEEP WRONG: node %zu, pixel %u %u\n", i, x0 + l % 8, y0 + l / 8);
                    }
                }
                if (i < res[l]) continue;
                ++awake[l];
                if (walk) {
                    // the filter first (rt_skip.hpp primary_filter_pass), then the reference's test on the sphere the stream carries
                    const Filt &f = filt[i];
                    const V3 v = sub(f.pc, eye);
                    const float bp = fmaf(v.z, dir[l].z, fmaf(v.y, dir[l].y, v.x * dir[l].x));
                    const bool pass = f.f5 <= bp;
                    if (f.rq > 0.0f) {                             // the lean BOUND step (rt_skip.hpp lean_bound_enters)
                        if (pass) cand = true;
                        if (pass && bp - f.rq < best[l]) enter = true; else res[l] = nd.skip;
                        continue;
                    }
                    float wdisc; const float wd = pass ? dist(f.pc, f.pr, eye, dir[l], &wdisc) : INFINITY;
                    if (pass) cand = true;
                    if (!nd.item) { if (!pass || wd >= best[l]) res[l] = nd.skip; else enter = true; }
                    else if (pass && !(wd >= best[l])) { best[l] = wd; bi[l] = (int)i; }
                    continue;
                }
                float disc; const float d = dist(nd.c, nd.r, eye, dir[l], &disc);
                if (disc >= 0) cand = true;
                if (disc >= 0 && !nd.item) {
                    const V3 v = sub(nd.c, eye); const float b = dot(v, dir[l]);
                    const float w = b - best[l];
                    const bool A = w < 0.0f;                      // best = INF: w = -INF
                    const float p = w * w, k = 1.0f + 0x1p-20f;
                    const bool N = !A && disc * k <= p;
                    const float q = fmaf(best[l], 0x1p-22f, w), r2 = q * q;
                    const bool G = !A && w <= best[l] && disc >= r2 * k;
                    if (!A && !N) undecided = true;
                    if (!A && !N && !G) undecided2 = true;
                    // sanity: the classification must agree with the reference's decision
                    const bool go = !(d >= best[l]);
                    if ((A && !go) || (N && go) || (G && !go)) { fprintf(stderr, "CLASSIFICATION WRONG %d %d %d go %d b %g best %g disc %g\n", A, N, G, go, b, best[l], disc); }
                }
                if (!nd.item) { if (d >= best[l]) res[l] = nd.skip; else enter = true; }
                else if (!(d >= best[l])) { best[l] = d; bi[l] = (int)i; }
            }
            if (nd.item) { if (cand) ++pI; else ++pLeafQ; ++i; continue; }
            if (!cand) { ++pQ; i = nd.skip; continue; }
            if (lean && filt[i].rq > 0.0f) { if (enter) ++pL1; else ++pL0; }
            if (!undecided) ++dec1; if (!undecided2) ++dec2;
            if (!enter) { ++pB0; if (!undecided) ++dec1_b0; i = nd.skip; continue; }
            if (tight) { ++pB1; ++i; continue; }      // un-fused: the own sphere is the ITEM step behind the BOUND
            // fused: the own sphere (next node) for the lanes that entered
            const Node &own = nodes[i + 1];
            bool ocand = false;
            for (unsigned l = 0; l < 64; ++l) {
                if (i + 1 < res[l]) continue;
                float disc; const float d = dist(own.c, own.r, eye, dir[l], &disc);
                if (disc >= 0) ocand = true;
                if (!(d >= best[l])) { best[l] = d; bi[l] = (int)(i + 1); }
            }
            if (ocand) ++pB2; else ++pB1;
            i += 2;
        }
        for (unsigned l = 0; l < 64; ++l) if (in[l]) hash = (hash ^ (uint64_t)(uint32_t)bi[l]) * 1099511628211ull;
        // shadow
        V3 sp[64]; bool need[64]; unsigned nn = 0;
        for (unsigned l = 0; l < 64; ++l) { need[l] = false; if (!in[l] || best[l] == INFINITY) continue; const Node &it = nodes[bi[l]]; const V3 nrm = normalized(add(eye, sub(mulf(dir[l], best[l]), it.c))); if (dot(nrm, light) >= 0) continue; sp[l] = add(add(eye, mulf(dir[l], best[l])), mulf(nrm, best[l] * sqrtf(1.1920929e-7f))); need[l] = true; ++nn; }
        if (!nn) continue;
        ++swaves;
        for (unsigned l = 0; l < 64; ++l) res[l] = need[l] ? 0u : 0xFFFFFFFFu;
        float q1[64], q2[64], ol[64];
        if (walk) for (unsigned l = 0; l < 64; ++l) {
            if (!need[l]) continue;
            const float x = sp[l].x - fq_m0[0], y = sp[l].y - fq_m0[1], z = sp[l].z - fq_m0[2];      // (rt_skip.hpp shadow_filter_origin; every origin is covered here)
            q1[l] = fmaf(z, fq_e1[2], fmaf(y, fq_e1[1], x * fq_e1[0])); q2[l] = fmaf(z, fq_e2[2], fmaf(y, fq_e2[1], x * fq_e2[0])); ol[l] = fmaf(z, fq_l[2], fmaf(y, fq_l[1], x * fq_l[0]));
        }
        for (size_t i = 0; i < n;) {
            const Node &nd = nodes[i];
            bool cand = false, enter = false, fin = false;
            ++wsteps;
            for (unsigned l = 0; l < 64; ++l) {
                if (i < res[l]) continue;
                ++awake[l];
                if (walk) {
                    // rt_skip.hpp shadow_filter_verdict<true>, then the reference's test of the tight ball for the lanes in between
                    const Filt &f = filt[i];
                    const float t0 = f.w1 - q1[l], t1 = f.w2 - q2[l], p2 = t0 * t0 + t1 * t1;
                    int verdict = 1;
                    if (p2 > f.r2o) verdict = 0;
                    else {
                        cand = true;
                        const float av = f.cl - ol[l], inn = fmaf(av, av, p2);
                        if (fmaf(inn, fq_k1, p2) <= f.r2i && (fq_a0 <= av || inn <= f.r2i)) verdict = 2;
                        else if (av <= -fq_a0 && f.r2o <= fq_kc * inn) verdict = 0;
                    }
                    float wdisc; const bool whit = verdict == 2 || (verdict == 1 && dist(nd.c, nd.r, sp[l], sdir, &wdisc) < INFINITY);
                    if (!nd.item) { if (!whit) res[l] = nd.skip; else enter = true; }
                    else if (verdict == 1 ? whit : dist(nd.c, nd.r, sp[l], sdir, &wdisc) < INFINITY) { res[l] = 0xFFFFFFFFu; fin = true; }
                    continue;
                }
                float disc; const bool hit = dist(nd.c, nd.r, sp[l], sdir, &disc) < INFINITY;
                if (disc >= 0) cand = true;
                if (!nd.item) { if (!hit) res[l] = nd.skip; else enter = true; }
                else if (hit) { res[l] = 0xFFFFFFFFu; fin = true; }
            }
            if (cand) ++sH; else ++sQ;
            if (!nd.item && enter) ++sEnt;      // (the fused walk tests the own sphere in this step: it saves the ITEM step behind it)
            size_t ni = (nd.item || enter) ? i + 1 : nd.skip;
            if (fin) { uint32_t m = 0xFFFFFFFFu; for (unsigned l = 0; l < 64; ++l) m = std::min(m, res[l] == 0xFFFFFFFFu ? 0xFFFFFFFFu : std::max<uint32_t>(res[l], (uint32_t)i + 1)); ni = m == 0xFFFFFFFFu ? n : m; }
            i = ni;
        }
        for (unsigned l = 0; l < 64; ++l) if (need[l]) hash = (hash ^ (res[l] == 0xFFFFFFFFu ? 1u : 2u)) * 1099511628211ull;
        wave_steps.push_back(wsteps);
        for (unsigned l = 0; l < 64; ++l) longest_px = std::max(longest_px, awake[l]);
    }
    std::sort(wave_steps.begin(), wave_steps.end(), [](uint32_t a, uint32_t b) { return a > b; });
    auto rank = [&](size_t k) { return k <= wave_steps.size() ? wave_steps[k - 1] : 0u; };
    printf("steps of the heaviest 8x8 wave (with a shadow walk) / rank 5 / rank 20 / rank 100 / rank 500: %u / %u / %u / %u / %u; longest single pixel (nodes its lane is awake at, both walks): %u\n",
           rank(1), rank(5), rank(20), rank(100), rank(500), longest_px);
    printf("%ux%u: %llu waves (%llu with shadow rays)\n", W, H, (unsigned long long)waves, (unsigned long long)swaves);
    printf("primary: quiet BOUND %llu, quiet ITEM %llu, BOUND cand/no enter %llu, BOUND enter/own quiet %llu, BOUND enter/own cand %llu, ITEM cand %llu\n", (unsigned long long)pQ, (unsigned long long)pLeafQ,
           (unsigned long long)pB0, (unsigned long long)pB1, (unsigned long long)pB2, (unsigned long long)pI);
    const double valu = 5.0 * (pQ + pLeafQ) + 25.0 * pB0 + 28.0 * pB1 + 42.0 * pB2 + 27.0 * pI;
    printf("primary VALU estimate: %.2f M (quiet %.2f, B0 %.2f, B1 %.2f, B2 %.2f, I %.2f)\n", valu / 1e6, 5.0 * (pQ + pLeafQ) / 1e6, 25.0 * pB0 / 1e6, 28.0 * pB1 / 1e6, 42.0 * pB2 / 1e6, 27.0 * pI / 1e6);
    printf("BOUND-cand steps decided by A/N alone: %llu (of which no-enter %llu), by A/N/G: %llu, of %llu\n", (unsigned long long)dec1, (unsigned long long)dec1_b0, (unsigned long long)dec2, (unsigned long long)(pB0 + pB1 + pB2));
    if (lean) {
        printf("lean: candidate BOUND steps %llu -- lean, nobody enters %llu; lean, entered %llu; the reference's test (no eye sphere) %llu; sleeping lanes the exact test makes winners %llu\n",
               (unsigned long long)(pB0 + pB1 + pB2), (unsigned long long)pL0, (unsigned long long)pL1, (unsigned long long)(pB0 + pB1 + pB2 - pL0 - pL1), (unsigned long long)lean_wrong);
        const double lv = valu - 20.0 * pL0 - 23.0 * pL1;
        printf("lean: primary VALU estimate %.2f M (a lean candidate BOUND step: 6 -- the quiet step's four, who is awake, b' - Rq and its compare)\n", lv / 1e6);
    }
    printf("steps: primary %llu, shadow %llu; hash of hit items and shadow verdicts %016llx\n", (unsigned long long)(pQ + pLeafQ + pB0 + pB1 + pB2 + pI), (unsigned long long)(sQ + sH), (unsigned long long)hash);
    // the shadow walk here always takes every node as a step of its own (the UN-FUSED walk); today's fused walk over the given bounds saves one per entered group
    if (!tight) printf("shadow steps of the FUSED walk (an entered group's own sphere tested in its BOUND step): %llu\n", (unsigned long long)(sQ + sH - sEnt));
    printf("shadow: quiet %llu, hit %llu -> VALU estimate %.2f M (6 / ~14)\n", (unsigned long long)sQ, (unsigned long long)sH, (6.0 * sQ + 14.0 * sH) / 1e6);
    return 0;
}
