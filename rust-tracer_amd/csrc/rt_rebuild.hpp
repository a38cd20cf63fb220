// rt_rebuild.hpp -- rt_sphere_order* / rt_scene_rebuild* (DESIGN.md 4.12): a dynamic scene's hierarchy rebuilt on the device from spheres
// in any order.  The topology of a dynamic scene never changes (rt_dynamic.hpp), so a rebuild is a PERMUTATION and a refit: the spheres
// are put in Morton order of their centres -- DFS slot k takes spheres[order[k]] -- and the groups, which span fixed slots, are refit
// over them.  Consecutive slots then hold neighbours in space, which is all a group of consecutive slots needs to be compact; with the
// ranges of rt_balanced_ranges (a topology that depends on the item count alone) the result is a median-split tree over the Morton curve.
//
// The key (include/rtrace_hip.h states it; rust_tracer_amd.sphere_keys restates it in numpy, bit for bit) is the ray key's origin part
// (rt_order.hpp) with 10 bits per axis instead of 3.  Everything in double -- an f32 sphere converts exactly -- with + - *, comparisons,
// truncation and powers of two only:
//   box     lo[a], hi[a] = min / max of the centres c[a] over the batch (radii take no part); ext = the largest hi[a] - lo[a]
//   scale   0 when ext == 0, else 2^(10 - e) with e = max(E - 1022, -1000), E the biased exponent field of ext: ext < 2^e
//   q[a]    trunc(clamp((c[a] - lo[a]) * scale, 0, 1023))
//   key     bit i of q[a] at bit 3i + a: 30 bits
// The sort is rt_order.hpp's, unchanged: k_sphere_keys leaves what k_ray_keys leaves (keys[0], the four digit histograms of the batch),
// so k_sort_plan skips the passes whose digit is constant -- every pass for a batch with one centre.  Whatever bits the spheres hold the
// keys are 32-bit integers and their stable sort is a permutation; k_gather_items still checks every index it reads.
#pragma once
#include "rt_order.hpp"
#include "rt_dynamic.hpp"

namespace rt {

__device__ __forceinline__ unsigned spread10(unsigned v)     // bit i of a 10-bit value to bit 3i
{
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// The box of the centres, as k_ray_box leaves the box of the origins: box->enc starts as zeroes, integer atomic max in any order.
template <typename T>
__global__ __launch_bounds__(kSortThreads) void k_sphere_box(const Item<T> *__restrict__ spheres, unsigned n, RayBox *box)
{
    unsigned long long m[6] = { 0, 0, 0, 0, 0, 0 };
    const unsigned long long stride = (unsigned long long)gridDim.x * kSortThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kSortThreads + threadIdx.x; i < n; i += stride) {
        const Item<T> it = spheres[i];                               // one 16- / 32-byte record
        const double c[3] = { (double)it.cx, (double)it.cy, (double)it.cz };
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned long long e = order_enc(c[a]);
            m[a] = ~e > m[a] ? ~e : m[a];
            m[3 + a] = e > m[3 + a] ? e : m[3 + a];
        }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long v = __shfl_xor(m[a], o, 64);
            m[a] = v > m[a] ? v : m[a];
        }
        if ((threadIdx.x & 63u) == 0u) atomicMax(&box->enc[a], m[a]);
    }
}

// One key per sphere (keys[i]) and, in totals[4][256], how often each value of each of the key's four bytes occurs in the batch.
template <typename T>
__global__ __launch_bounds__(kSortThreads) void k_sphere_keys(const Item<T> *__restrict__ spheres, unsigned n, const RayBox *__restrict__ box,
                                                              unsigned *__restrict__ keys, unsigned *totals)
{
    __shared__ unsigned h[4 * 256];
    for (unsigned k = threadIdx.x; k < 4 * 256; k += kSortThreads) h[k] = 0;
    __syncthreads();
    const double lx = order_dec(~box->enc[0]), ly = order_dec(~box->enc[1]), lz = order_dec(~box->enc[2]);
    const double ex = order_dec(box->enc[3]) - lx, ey = order_dec(box->enc[4]) - ly, ez = order_dec(box->enc[5]) - lz;
    double ext = ex;
    if (ey > ext) ext = ey;
    if (ez > ext) ext = ez;
    int e = (int)(((unsigned long long)__double_as_longlong(ext) >> 52) & 0x7FFull) - 1022;
    if (e < -1000) e = -1000;
    const double scale = ext > 0.0 ? __longlong_as_double((long long)(1023 + 10 - e) << 52) : 0.0;      // (E <= 2047: the field stays >= 8)
    const unsigned long long stride = (unsigned long long)gridDim.x * kSortThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kSortThreads + threadIdx.x; i < n; i += stride) {
        const Item<T> it = spheres[i];
        const unsigned qx = clamp_trunc(((double)it.cx - lx) * scale, 1023.0), qy = clamp_trunc(((double)it.cy - ly) * scale, 1023.0),
                       qz = clamp_trunc(((double)it.cz - lz) * scale, 1023.0);
        const unsigned key = spread10(qx) | (spread10(qy) << 1) | (spread10(qz) << 2);
        keys[i] = key;
#pragma unroll
        for (unsigned p = 0; p < 4; ++p) atomicAdd(&h[p * 256 + ((key >> (8 * p)) & 255u)], 1u);
    }
    __syncthreads();
    for (unsigned k = threadIdx.x; k < 4 * 256; k += kSortThreads)
        if (h[k]) atomicAdd(&totals[k], h[k]);
}

// dst[k] = src[order[k]]: the spheres into DFS order, a whole record per thread.  An index that is no index (the sort leaves none)
// reads the slot's own sphere.
template <typename T>
__global__ __launch_bounds__(kBlockThreads) void k_gather_items(const Item<T> *__restrict__ src, const unsigned *__restrict__ order, unsigned n,
                                                                Item<T> *__restrict__ dst)
{
    const unsigned k = blockIdx.x * kBlockThreads + threadIdx.x;
    if (k >= n) return;
    const unsigned i = order[k];
    dst[k] = src[i < n ? i : k];
}

}  // namespace rt
