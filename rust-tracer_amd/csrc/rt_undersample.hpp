// rt_undersample.hpp -- rt_render_camera_undersampled*: the camera frame of rt_trace.hpp sampled once per step x step cell, and the
// refinement of such a frame to half the step in place.
//
// The lattice of a step s is every pixel with x % s == 0 and y % s == 0, anchored at the image origin; cell (cx, cy) is the pixels
// [cx*s, cx*s + s) x [cy*s, cy*s + s) and holds F(cx*s, cy*s), the camera kernel's pixel.  A lane traces its cell's anchor with
// trace_ray / accumulate / scale_u8 of rt_trace.hpp -- the arithmetic of a sample is the camera kernel's by construction -- and the
// wave then fills the cells' parts inside the tile.
//
// Work mapping (one lane per TRACED cell; `tiles` carries blk_first / blks_x in units of the blocks below):
//   fresh   (refine == 0)  a workgroup of 256 is 16 x 16 cells of the tile's cell grid, an 8 x 8 patch per wave (the camera kernel's
//                          layout with cells for pixels).
//   refine  (refine == 1)  the buffer holds the step-2s frame.  A step-s cell whose anchor lies on the 2s lattice is child (0, 0) of
//                          its 2s cell: already correct, neither traced nor written.  A workgroup of 192 is 8 x 8 cells of the 2s
//                          grid; thread n takes parent n / 3 (row-major in the 8 x 8) and its child n % 3 + 1 = (1,0), (0,1), (1,1):
//                          three full waves, each over about three rows of parents (16 x 6 step-s cells).
// A cell that does not meet the tile has a dead lane; a cell whose anchor lies outside the tile is traced from the anchor all the same.
//
// Fill: wave-cooperative.  Lanes form groups of P = min(64, Pw * Pw), Pw = the power of two >= s; in round `it` group g serves the cell
// of lane it * (64 / P) + g (word, first index and clipped size arrive by ds_bpermute) and its P lanes, laid out Pw wide, store the
// cell's rows -- s = 1: every lane its own pixel, s = 2: 16 cells a round, s >= 33: a round is 64 contiguous words of one cell row.
#pragma once
#include "rt_trace.hpp"

namespace rt {

template <typename T> struct UnderArgs {
    TraceArgs<T> t;             // the camera flavour's arguments; t.tiles: blk_first / blks_x count the blocks described above
    uint32_t step;              // s
    uint32_t refine;            // 0: every cell traced and written; 1: the buffer holds the step-2s frame
    uint32_t lg_pw, lg_p;       // log2 Pw, log2 P
};

template <typename T, bool COUNT>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(COUNT ? 4 : 8))) void k_trace_undersampled(UnderArgs<T> a)
{
    // the block's tile: the last one whose first block is <= blockIdx.x (block-uniform)
    unsigned lo = 0, hi = a.t.n - 1;
    while (lo < hi) {
        const unsigned mid = (lo + hi + 1) >> 1;
        if (a.t.tiles[mid].blk_first <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const TileDev tile = a.t.tiles[lo];
    const unsigned lb = blockIdx.x - tile.blk_first;
    const unsigned bx = lb % tile.blks_x, by = lb / tile.blks_x;
    const unsigned s = a.step;
    unsigned cx, cy;
    if (a.refine == 0u) {
        const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        cx = tile.l / s + bx * kBlockW + (wave & 1) * 8u + (lane & 7u);
        cy = tile.b / s + by * kBlockH + (wave >> 1) * 8u + (lane >> 3);
    } else {
        const unsigned p = threadIdx.x / 3u, q = threadIdx.x - 3u * p + 1u;
        cx = 2u * (tile.l / (2u * s) + bx * 8u + (p & 7u)) + (q & 1u);
        cy = 2u * (tile.b / (2u * s) + by * 8u + (p >> 3)) + (q >> 1);
    }
    // the anchor; the cell is live when it meets the tile (its clipped extent is formed after the walks: nothing of it lives across them)
    // (the anchor of a live cell fits 16 bits, as the image does: one register holds both across the walks)
    const bool inside = cx * s + s > tile.l && cx * s < tile.r && cy * s + s > tile.b && cy * s < tile.t;
    const unsigned xy = (cx * s) | ((cy * s) << 16);
    if (__ballot(inside) == 0) return;          // (waves are independent: no LDS, no barrier)
    TraceCounts c;
    const unsigned spp = a.t.spp;
    const T ssf = T(spp);
    const T total_recip = T(1.0) / (ssf * ssf);
    const T fw = T(a.t.width), fh = T(a.t.height);
    const T half_w = fw / T(2.0), half_h = fh / T(2.0);
    const V3<T> eye = { a.t.cam[0], a.t.cam[1], a.t.cam[2] };
    V3<T> g = { T(0.0), T(0.0), T(0.0) };
    T alpha = T(0.0);
    for (unsigned ssx = 0; ssx < spp; ++ssx) {
        for (unsigned ssy = 0; ssy < spp; ++ssy) {
            unsigned xy_here = xy;
            asm volatile("" : "+v"(xy_here));                    // (unpacked here, sample by sample: hoisted, x and y cost the f64 flavour a spill)
            const unsigned x = xy_here & 0xFFFFu, y = xy_here >> 16;
            const T xres = T(x) + T(ssx) / ssf;                  // render.rs:238-242, as k_trace_rays
            const T yres = T(y) + T(ssy) / ssf;
            const T u = xres - half_w, v = (fh - yres) - half_h;
            const V3<T> dir = normalized(V3<T>{ (a.t.cam[3] * u + a.t.cam[6] * v) + a.t.cam[9] * fw,
                                                (a.t.cam[4] * u + a.t.cam[7] * v) + a.t.cam[10] * fw,
                                                (a.t.cam[5] * u + a.t.cam[8] * v) + a.t.cam[11] * fw });
            T gdot;
            const uint8_t state = trace_ray<T, COUNT>(a.t, eye, dir, inside, gdot, c);
            if (inside) alpha += accumulate(g, state, gdot);
        }
    }
    unsigned rgba = 0u;                         // spp == 0: the reference's black pixel
    if (spp != 0u) {
        g = mulf(g, total_recip);               // render.rs:251-253
        alpha *= total_recip;
        rgba = scale_u8(g.x) | (scale_u8(g.y) << 8) | (scale_u8(g.z) << 16) | (scale_u8(alpha) << 24);
    }
    // ---------------- fill ----------------
    unsigned *const out = reinterpret_cast<unsigned *>(a.t.out);
    const unsigned pitch = (unsigned)tile.r - tile.l;
    const unsigned x = xy & 0xFFFFu, y = xy >> 16, lane = __lane_id();
    const unsigned x0 = max(x, (unsigned)tile.l), x1 = min(x + s, (unsigned)tile.r);
    const unsigned y0 = max(y, (unsigned)tile.b), y1 = min(y + s, (unsigned)tile.t);
    const unsigned first = inside ? (unsigned)out_index(tile, x0, y0, 0) : 0u;      // (a pass holds < 2^32 pixels)
    const unsigned cw = inside ? x1 - x0 : 0u, ch = inside ? y1 - y0 : 0u;
    const unsigned lg_pw = a.lg_pw, lg_p = a.lg_p;
    const unsigned pw = 1u << lg_pw, ph = 1u << (lg_p - lg_pw), rounds = 1u << lg_p;
    const unsigned grp = lane >> lg_p, sub = lane & (rounds - 1u);
    const unsigned col0 = sub & (pw - 1u), row0 = sub >> lg_pw;
    for (unsigned it = 0; it < rounds; ++it) {
        const int src = (int)(it * (64u >> lg_p) + grp);
        const unsigned w_src = (unsigned)__shfl((int)cw, src, 64), h_src = (unsigned)__shfl((int)ch, src, 64);
        const unsigned first_src = (unsigned)__shfl((int)first, src, 64), word = (unsigned)__shfl((int)rgba, src, 64);
        for (unsigned row = row0; row < h_src; row += ph)
            for (unsigned col = col0; col < w_src; col += pw)
                out[(size_t)first_src + (size_t)row * pitch + col] = word;
    }
    if constexpr (COUNT) {
        const unsigned long long prim = wave_sum(inside ? spp * spp : 0u), hits = wave_sum(c.hits), sh = wave_sum(c.shadow), oc = wave_sum(c.occ);
        const unsigned long long its = wave_sum(c.items), bds = wave_sum(c.bounds), ptot = wave_sum(c.ptests);
        if (lane == 0u) {
            Counters *const stripe = a.t.counters + blockIdx.x % kCounterStripes;
            atomicAdd(&stripe->primary, prim);
            atomicAdd(&stripe->hits, hits);
            atomicAdd(&stripe->shadow, sh);
            atomicAdd(&stripe->occluded, oc);
            atomicAdd(&stripe->sphere_tests, its);
            atomicAdd(&stripe->bound_tests, bds);
            atomicAdd(&stripe->primary_tests, ptot);
        }
    }
}

}  // namespace rt
